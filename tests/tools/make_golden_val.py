"""Generate tests/golden/val_ref.npz by RUNNING THE REFERENCE's validation pass (development container only):

    python tests/tools/make_golden_val.py

train.py's `test_acc` (train.py:27-106) on six tiny synthetic frames (2048 points, 160 x 512 image, name-keyed synthetic weights,
model.eval(), mode='val'), plus the same call on the first three of them (the fixed-6-rows quirk of train.py:31,103), the fine recall of
train.py:268-280 and the pc_score scalars of train.py:256-259 on every frame's outputs.

`acc` comes from the reference's own function: train.py is imported with stubs for the third-party modules that are absent here
(tensorboard, and the dataset modules whose imports need cv2 / open3d / torchvision) - its `__main__` guard keeps the script part
from running - and `test_acc` is called on a list of DataLoader-shaped batches.  It returns only `acc`; the per-frame `counts` and
`n_true` are obtained by evaluating its statements :72-101 verbatim on the same tensors, and the generator asserts that train.py:103 on
those counts is bit-equal to what the function returned.

Counting is rank-based, so the fixture must be WELL CONDITIONED: an implementation whose descriptors differ from the reference's by
rounding has to find the same ranks.  Checked in the reference's own float64 evaluation (the same module in double precision), per frame:
  * within every row of dist the six smallest values are pairwise either equal to within 0 ulp (duplicate key points) or further apart
    than common.TIE (1e-5),
  * no projected distance lies within 1e-3 of opt.dist_thres,
  * the two largest of every key point's 16 fine cosine similarities are further apart than TIE.
A frame's label seed is redrawn until the reference alone satisfies this (and, for up to 60 draws, until the frame has a non-zero
top-1 count: the generator asserts that at least one frame does); the seeds are recorded.  Key points are drawn with
replacement, and the generator asserts that at least one frame's pc_kpt_idx holds duplicates (membership in test_acc is by VALUE).

The fixture is data: labels, input hashes and the reference's results, nothing else."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
GOLD = os.path.join(ROOT, "tests", "golden")

import ref_shims  # noqa: E402
from common import TIE  # noqa: E402
from make_golden import build_reference_model, frame_inputs, sha  # noqa: E402

NUM_KPT = 32
FRAME_IDS = (1, 2, 3, 4, 5, 6)
NUM_POINTS, PYR_SEED = 2048, 11
MARGIN_PX = 1e-3
MAX_DRAWS = 400
TOP1_DRAWS = 60   # draws spent per frame looking for a well-conditioned label set with a non-zero top-1 count


def import_train():
    """the reference's train module, with stubs for what its top-level imports cannot find in this container"""
    import importlib

    ref_shims.import_reference()
    tb = types.ModuleType("torch.utils.tensorboard")
    tb.SummaryWriter = object
    sys.modules.setdefault("torch.utils.tensorboard", tb)
    for name, cls in (("data.kitti", "kitti_pc_img_dataset"), ("data.nuscenes", "nuscenes_pc_img_dataset")):
        if name not in sys.modules:
            m = types.ModuleType(name)
            setattr(m, cls, object)
            sys.modules[name] = m
    return importlib.import_module("train")


def make_labels(points4: np.ndarray, n1: int, seed: int):
    """A data/kitti.py:305-420-shaped label set for a tiny frame, key points drawn WITH replacement (as the reference's sampling does
    when a frame has fewer candidates than num_kpt)."""
    g = np.random.default_rng(seed)
    K_4 = np.array([[20.0, 0.0, 32.0], [0.0, 20.0, 10.0], [0.0, 0.0, 1.0]], dtype=np.float32)
    ang = 0.05
    P = np.eye(4, dtype=np.float32)
    P[:3, :3] = np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]], dtype=np.float32)
    P[:3, 3] = [0.3, -0.1, 0.5]
    cam = points4 @ P[:3, :3].T + P[:3, 3]
    uvw = cam @ K_4.T
    u, v = uvw[:, 0] / uvw[:, 2], uvw[:, 1] / uvw[:, 2]
    inside = (cam[:, 2] > 0.5) & (u >= 0) & (u < 64) & (v >= 0) & (v < 20)
    inl, outl = np.nonzero(inside)[0], np.nonzero(~inside)[0]
    assert len(inl) >= 8 and len(outl) >= 8, (len(inl), len(outl))
    pc_kpt_idx = g.choice(inl, NUM_KPT, replace=True)
    pc_outline_idx = g.choice(outl, NUM_KPT, replace=True)
    pu = np.clip(np.floor(u[pc_kpt_idx]) + g.integers(-1, 2, NUM_KPT), 0, 63)
    pv = np.clip(np.floor(v[pc_kpt_idx]) + g.integers(-1, 2, NUM_KPT), 0, 19)
    coarse_img_kpt_idx = (pv * 64 + pu).astype(np.int64)
    fine_center = np.stack([g.integers(2, 254, NUM_KPT), g.integers(2, 78, NUM_KPT)]).astype(np.int64)   # (x, y) on the 1/2 map
    fine_xy = fine_center + g.integers(-2, 2, (2, NUM_KPT))
    fine_inl = g.integers(0, n1, NUM_KPT).astype(np.int64)
    return dict(K_4=K_4, P=P, pc_kpt_idx=pc_kpt_idx.astype(np.int64), pc_outline_idx=pc_outline_idx.astype(np.int64),
                coarse_img_kpt_idx=coarse_img_kpt_idx, fine_center_kpt_coors=fine_center, fine_xy=fine_xy, fine_pc_inline_index=fine_inl)


class OptK:
    """the options the statements read"""

    def __init__(self, opt):
        self.num_kpt, self.dist_thres = NUM_KPT, opt.dist_thres


def coarse_statements(img_features, pc_features, points4, lab, opt, topk_range=5):
    """train.py:63-66 and :72-101 verbatim on loaded tensors (one frame) -> dist_corr, correspondence_mask, the projected pixel distances,
    this frame's count row and its true_value_list."""
    pc_kpt_idx, coarse_img_kpt_idx, K_4, P = lab["pc_kpt_idx"], lab["coarse_img_kpt_idx"], lab["K_4"], lab["P"]
    pc_data_dict = {"points": [None, points4]}
    H8, W8 = img_features.shape[2:]
    img_x = torch.linspace(0, W8 - 1, W8).view(1, -1).expand(H8, W8).unsqueeze(0)
    img_y = torch.linspace(0, H8 - 1, H8).view(-1, 1).expand(H8, W8).unsqueeze(0)
    img_xy = torch.cat((img_x, img_y), dim=0).to(img_features.dtype)
    pc_features_inline = torch.gather(pc_features, index=pc_kpt_idx.expand(pc_features.size(0), opt.num_kpt), dim=-1)
    pc_xyz_inline = torch.gather(pc_data_dict['points'][-1].T, index=pc_kpt_idx.unsqueeze(0).expand(3, opt.num_kpt), dim=-1)
    img_features_flatten = img_features.contiguous().view(img_features.size(1), -1)
    img_xy_flatten = img_xy.contiguous().view(2, -1)
    img_features_flatten_inline = torch.gather(img_features_flatten, index=coarse_img_kpt_idx.unsqueeze(0).expand(img_features_flatten.size(0), opt.num_kpt), dim=-1)
    img_xy_flatten_inline = torch.gather(img_xy_flatten, index=coarse_img_kpt_idx.unsqueeze(0).expand(2, opt.num_kpt), dim=-1)
    pc_xyz_projection = torch.mm(K_4, (torch.mm(P[0:3, 0:3], pc_xyz_inline) + P[0:3, 3:]))
    pc_xy_projection = pc_xyz_projection[0:2, :] / pc_xyz_projection[2:, :]
    pix_dist = torch.sqrt(torch.sum(torch.square(img_xy_flatten_inline.unsqueeze(-1) - pc_xy_projection.unsqueeze(-2)), dim=0))
    correspondence_mask = (pix_dist <= opt.dist_thres).float()
    dist_corr = 1 - torch.sum(img_features_flatten_inline.unsqueeze(-1) * pc_features_inline.unsqueeze(-2), dim=0)
    dist_mask = correspondence_mask.to(dist_corr.dtype) * dist_corr
    true_index_list = torch.nonzero(dist_mask, as_tuple=False)
    true_value_list = dist_mask[true_index_list[:, 0], true_index_list[:, 1]].tolist()
    sorted_dist, indices = torch.sort(dist_corr, dim=-1, descending=False)
    row = torch.zeros(topk_range)
    for k in range(1, topk_range + 1):
        candidate_values = sorted_dist[:, 0:k]
        for i in range(pc_kpt_idx.shape[0]):
            candidates = candidate_values[i, :].tolist()
            for candidate in candidates:
                if candidate in true_value_list:
                    row[k - 1] += 1
    return dist_corr, correspondence_mask, pix_dist, row, true_value_list


def fine_statements(fine_img_feature_patch, fine_pc_inline_feature, lab):
    """train.py:268-279 verbatim -> the cosine matrix (K, 16) and the number of recalled key points"""
    from einops import rearrange

    relative_coors = lab["fine_xy"] - lab["fine_center_kpt_coors"] + 2
    relative_index = relative_coors[1, :] * 4 + relative_coors[0, :]
    recall_num = torch.zeros(NUM_KPT)
    fine_pc_inline = fine_pc_inline_feature.unsqueeze(-1)
    fine_img_feature_flatten = torch.squeeze(rearrange(fine_img_feature_patch, 'b c h w -> b c (h w)'))
    fine_dist = torch.cosine_similarity(fine_img_feature_flatten.unsqueeze(-1), fine_pc_inline.unsqueeze(-2))
    fine_dist = torch.squeeze(fine_dist)
    fine_predict_index = torch.argmax(fine_dist, dim=1)
    mask = torch.where(fine_predict_index == relative_index)[0]
    recall_num[mask] = 1
    return fine_dist, int(torch.sum(recall_num)), fine_predict_index


def score_statements(coarse_pc_score, lab):
    """train.py:256-259"""
    s_in = torch.squeeze(coarse_pc_score[:, :, lab["pc_kpt_idx"]])
    s_out = torch.squeeze(coarse_pc_score[:, :, lab["pc_outline_idx"]])
    return np.array([float(s_in.max()), float(s_in.min()), float(torch.mean(s_in)), float(s_out.max()), float(s_out.min()), float(torch.mean(s_out))], dtype=np.float32)


def well_conditioned(dist64, pix64, cos64, dist_thres):
    """the three conditions of the module docstring, on float64 tensors -> (ok, reason)"""
    s = torch.sort(dist64, dim=-1).values[:, :6]
    for a in range(6):
        for b in range(a + 1, 6):
            gap = (s[:, b] - s[:, a]).abs()
            bad = (gap != 0) & (gap <= TIE)
            if bool(bad.any()):
                return False, "row gap %.3g" % float(gap[bad].min())
    if bool(((pix64 - dist_thres).abs() <= MARGIN_PX).any()):
        return False, "projected distance near the threshold"
    top2 = torch.sort(cos64, dim=1, descending=True).values[:, :2]
    if bool(((top2[:, 0] - top2[:, 1]) <= TIE).any()):
        return False, "fine cosine tie"
    return True, ""


def dbl(t):
    return t.double() if torch.is_tensor(t) and t.is_floating_point() else t


def main():
    torch.manual_seed(0)
    net, model, sd = build_reference_model("gn")
    train = import_train()
    ref_opt = ref_shims.reference_options()
    opt = OptK(ref_opt)
    torch.set_default_dtype(torch.float64)
    _, model64, _ = build_reference_model("gn")
    model64 = model64.double().eval()
    torch.set_default_dtype(torch.float32)
    model.eval()
    out = {"frame_ids": np.array(FRAME_IDS), "num_points": NUM_POINTS, "pyr_seed": PYR_SEED, "num_kpt": NUM_KPT, "dist_thres": opt.dist_thres,
           "tie": TIE, "margin_px": MARGIN_PX}
    frames, batches, seeds, any_dup = [], [], [], False
    counts, n_true, fine_hits, stats = [], [], [], []
    for fi, frame_id in enumerate(FRAME_IDS):
        fr, data = frame_inputs(frame_id, NUM_POINTS, PYR_SEED)
        img = torch.from_numpy(fr.img)[None]
        n1 = data["points"][1].shape[0]
        data64 = {k: ([dbl(t) for t in v] if isinstance(v, list) else dbl(v)) for k, v in data.items()}
        coarse64, fallback = None, None
        for draw in range(MAX_DRAWS):
            seed = 1000 * frame_id + draw
            lab_np = make_labels(data["points"][-1].numpy(), n1, seed)
            lab = {k: torch.from_numpy(v) for k, v in lab_np.items()}
            lab64 = {k: dbl(v) for k, v in lab.items()}
            with torch.no_grad():
                # the float64 forward: its coarse outputs do not depend on the labels, its fine outputs are two gathers from label-independent maps
                if coarse64 is None:
                    taps = {}
                    h1 = model64.pc_encoder.register_forward_hook(lambda m, i, o: taps.__setitem__("pc_set", o))
                    h2 = model64.img_upsample_2.register_forward_hook(lambda m, i, o: taps.__setitem__("up2", o))
                    o64 = model64(data64, img.double(), lab["fine_center_kpt_coors"], lab["fine_xy"], lab["fine_pc_inline_index"], "val")
                    h1.remove(), h2.remove()
                    coarse64 = (o64[0], o64[1])
                    fine_map64 = torch.nn.functional.normalize(taps["up2"], dim=1, p=2)          # network.py:130
                    fine_pts64 = torch.nn.functional.normalize(taps["pc_set"][-4], dim=1, p=2)   # network.py:83
                    assert torch.equal(o64[5], fine_pts64[lab["fine_pc_inline_index"]])
                    assert torch.equal(o64[4], torch.squeeze(net.extract_patch(fine_map64, lab["fine_center_kpt_coors"])))
                patch64 = torch.squeeze(net.extract_patch(fine_map64, lab["fine_center_kpt_coors"]))   # network.py:141
                fpc64 = fine_pts64[lab["fine_pc_inline_index"]]                                         # network.py:138
                d64, _m64, pix64, _row64, _tv64 = coarse_statements(coarse64[0], coarse64[1], data64["points"][-1], lab64, opt)
                cos64, _h64, _p64 = fine_statements(patch64, fpc64, lab)
            ok, why = well_conditioned(d64, pix64, cos64, opt.dist_thres)
            if ok and fallback is None:
                fallback = seed
            # ... and a fixture whose top-1 counts are all zero would not notice a lost first candidate: prefer a label set with top-1 hits
            if ok and (float(_row64[0]) > 0 or draw >= TOP1_DRAWS):
                break
            if not ok:
                print("frame %d seed %d rejected: %s" % (frame_id, seed, why))
        else:
            raise AssertionError("frame %d: no well-conditioned label set in %d draws" % (frame_id, MAX_DRAWS))
        seeds.append(seed)
        any_dup |= len(np.unique(lab_np["pc_kpt_idx"])) < NUM_KPT
        with torch.no_grad():   # the reference's fp32 evaluation with the accepted labels: what the fixture records
            o32 = model(data, img, lab["fine_center_kpt_coors"], lab["fine_xy"], lab["fine_pc_inline_index"], "val")
            d32, m32, _pix32, row, tv = coarse_statements(o32[0], o32[1], data["points"][-1], lab, opt)
            _cos32, hits, pred = fine_statements(o32[4], o32[5], lab)
        assert torch.equal(m32, _m64), "fp32 and fp64 masks differ"
        assert torch.equal(pred, _p64), "fp32 and fp64 fine picks differ"
        counts.append(row.numpy().astype(np.int32)), n_true.append(len(tv)), fine_hits.append(hits), stats.append(score_statements(o32[3], lab))
        out["sha_points_%d" % fi], out["sha_img_%d" % fi], out["sha_feats_%d" % fi] = sha(fr.points), sha(fr.img), sha(fr.feats)
        for k, v in lab_np.items():
            out["lab%d_%s" % (fi, k)] = v
        out["dist_%d" % fi], out["mask_%d" % fi] = d32.numpy(), m32.numpy()
        # a DataLoader-shaped batch (batch size 1) for the reference's own function
        pcd = {k: [t[None].clone() for t in data[k]] for k in ("points", "neighbors", "subsampling", "upsampling")}
        pcd["feats"] = data["feats"][None].clone()
        batches.append({"img": img.clone(), "pc_data_dict": pcd, "K": lab["K_4"][None], "K_4": lab["K_4"][None], "P": lab["P"][None],
                        "coarse_img_mask": torch.zeros(1, 20, 64), "pc_kpt_idx": lab["pc_kpt_idx"][None], "pc_outline_idx": lab["pc_outline_idx"][None],
                        "fine_img_kpt_index": torch.zeros(1, NUM_KPT, dtype=torch.int64), "coarse_img_kpt_idx": lab["coarse_img_kpt_idx"][None],
                        "fine_center_kpt_coors": lab["fine_center_kpt_coors"][None], "fine_xy_coors": lab["fine_xy"][None],
                        "fine_pc_inline_index": lab["fine_pc_inline_index"][None]})
        print("frame %d: seed %d, n_true %d, counts %s, fine hits %d" % (frame_id, seed, len(tv), row.tolist(), hits))
    assert any_dup, "no frame's pc_kpt_idx holds duplicates"
    counts, n_true = np.stack(counts), np.array(n_true, dtype=np.int32)
    assert (counts[:, 0] > 0).any(), "every frame's top-1 count is zero"

    def clone_batches(bs):
        return [{k: ({kk: ([t.clone() for t in vv] if isinstance(vv, list) else vv.clone()) for kk, vv in v.items()} if isinstance(v, dict) else v.clone())
                 for k, v in b.items()} for b in bs]

    for name, nb in (("acc", 6), ("acc3", 3)):
        with torch.no_grad():
            acc = train.test_acc("cpu", model, clone_batches(batches[:nb]), opt)    # train.py:308
        topk_list = torch.zeros(6, 5)
        topk_list[:nb] = torch.from_numpy(counts[:nb]).float()
        assert torch.equal(acc, torch.mean(topk_list / int(n_true[nb - 1]), dim=0)), (acc, counts, n_true)   # train.py:103 on the recorded counts
        out[name] = acc.numpy()
        print(name, acc.tolist())
    out.update(counts=counts, n_true=n_true, fine_hits=np.array(fine_hits, dtype=np.int32), score_stats=np.stack(stats), label_seeds=np.array(seeds))
    np.savez_compressed(os.path.join(GOLD, "val_ref.npz"), **out)
    print("val_ref.npz: %d arrays, %d bytes" % (len(out), os.path.getsize(os.path.join(GOLD, "val_ref.npz"))))


if __name__ == "__main__":
    main()
