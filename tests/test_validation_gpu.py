"""The validation pass on the GPU (cofii2p_amd.validation, csrc/validation.hip): the monitors kernel against the reference's torch
expressions and counting rule, the stack-mode mode='val' forward against single-frame forwards, `validate()` against the reference's own
`test_acc` (tests/golden/val_ref.npz), and the monitors of a recorded training step.  Needs a real MI355X."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from common import frame_inputs, load_golden, sha  # noqa: E402

DEV = "cuda:0"


class Opt:
    img_H, img_W, img_fine_resolution_scale, norm = 160, 512, 32, "gn"


class VOpt:
    dist_thres, pos_margin, neg_margin = 1.0, 0.2, 1.8


@pytest.fixture(scope="module")
def model():
    from cofii2p_amd import ops
    from cofii2p_amd.network import CoFiI2P

    saved, ops.GEMM_MODE = ops.GEMM_MODE, "f32"   # as tests/test_forward_gpu.py: fp32 tolerances against the reference
    yield CoFiI2P(Opt()).to(DEV)
    ops.GEMM_MODE = saved


# ------------------------------------------------------------------------------------------ (a) the kernel
def count_by_value(dist, mask, topk=5):
    """test_acc's counting rule (train.py:89-101) on one frame's (K, K) CPU tensors, host side: the true values are the distances of the
    masked entries that are not zero; every row contributes its `topk` smallest distances as candidates; counts[k - 1] = candidates among
    the first k of a row that EQUAL some true value, wherever in the matrix that value sits -> (counts, number of true values)"""
    picked = (mask * dist) != 0
    true_values = set(dist[picked].tolist())
    ranked = torch.sort(dist, dim=1).values[:, :topk].tolist()
    per_rank = [sum(row[p] in true_values for row in ranked) for p in range(topk)]
    return [sum(per_rank[:k]) for k in range(1, topk + 1)], int(picked.sum())


def _random_case(B, K, seed, idt=torch.int64):
    g = torch.Generator().manual_seed(seed)
    C, H8, W8, N4, C2 = 128, 20, 64, 160, 64
    T = H8 * W8
    img_desc = torch.nn.functional.normalize(torch.randn(B, C, T, generator=g), dim=1)
    pc_desc = torch.nn.functional.normalize(torch.randn(B, C, N4, generator=g), dim=1)
    K_4 = torch.tensor([[20.0, 0.0, 32.0], [0.0, 20.0, 10.0], [0.0, 0.0, 1.0]]).repeat(B, 1, 1)
    P = torch.eye(4).repeat(B, 1, 1)
    P[:, :3, 3] = torch.tensor([0.3, -0.1, 0.5]) + 0.05 * torch.randn(B, 3, generator=g)
    # points in front of the camera that project into the 64 x 20 map
    z = 4.0 + 6.0 * torch.rand(B, N4, generator=g)
    u, v = 1.0 + 62.0 * torch.rand(B, N4, generator=g), 1.0 + 18.0 * torch.rand(B, N4, generator=g)
    cam = torch.stack([(u - 32.0) / 20.0 * z, (v - 10.0) / 20.0 * z, z], -1)
    points4 = (cam - P[:, None, :3, 3]).reshape(B * N4, 3).contiguous()
    # key points drawn WITH replacement from a small pool: duplicates in every frame
    pool = torch.randint(0, N4, (B, max(4, K // 2)), generator=g)
    pc_kpt = torch.gather(pool, 1, torch.randint(0, pool.shape[1], (B, K), generator=g))
    pu = (torch.gather(u, 1, pc_kpt).floor() + torch.randint(-1, 2, (B, K), generator=g)).clamp(0, W8 - 1)
    pv = (torch.gather(v, 1, pc_kpt).floor() + torch.randint(-1, 2, (B, K), generator=g)).clamp(0, H8 - 1)
    img_kpt = (pv * W8 + pu).long()
    for f in range(B):   # matched pairs get near descriptors, so that true values sit among the smallest of their rows
        for k in range(0, K, 2):
            img_desc[f, :, img_kpt[f, k]] = torch.nn.functional.normalize(pc_desc[f, :, pc_kpt[f, k]] + 0.05 * torch.randn(C, generator=g), dim=0)
    pc_out = torch.randint(0, N4, (B, K), generator=g)
    pc_score = torch.rand(B * N4, generator=g)
    patches = torch.nn.functional.normalize(torch.randn(B, K, C2, 16, generator=g), dim=2)
    fine_pc = torch.nn.functional.normalize(torch.randn(B, K, C2, generator=g), dim=2)
    center = torch.stack([torch.randint(2, 254, (B, K), generator=g), torch.randint(2, 78, (B, K), generator=g)], 1)
    fine_xy = center + torch.randint(-2, 2, (B, 2, K), generator=g)
    rel = (fine_xy[:, 1] - center[:, 1] + 2) * 4 + (fine_xy[:, 0] - center[:, 0] + 2)
    for f in range(B):   # every third key point: the labelled pixel carries the point's descriptor -> a hit
        for k in range(0, K, 3):
            patches[f, k, :, rel[f, k]] = fine_pc[f, k]
    lab = {"pc_kpt_idx": pc_kpt, "pc_outline_idx": pc_out, "coarse_img_kpt_idx": img_kpt, "fine_xy": fine_xy, "fine_center_kpt_coors": center}
    D = lambda t: t.to(DEV).contiguous()
    return dict(img_desc=D(img_desc), pc_desc=D(pc_desc), W8=W8, points4=D(points4), pc_score=D(pc_score), patches=D(patches), fine_pc=D(fine_pc),
                lab={k: D(v.to(idt)) for k, v in lab.items()}, K_4=D(K_4), P=D(P))


def _torch_expressions(c, f, K):
    """train.py:72-86 and :256-257 on frame f of a case, on the device in fp32 (dist also in fp64)"""
    lab = {k: v[f].long() for k, v in c["lab"].items()}
    img_features, pc_features = c["img_desc"][f], c["pc_desc"][f]
    N4 = pc_features.shape[1]
    pts = c["points4"][f * N4:(f + 1) * N4]
    W8 = c["W8"]
    H8 = img_features.shape[1] // W8
    img_x = torch.linspace(0, W8 - 1, W8, device=DEV).view(1, -1).expand(H8, W8).unsqueeze(0)
    img_y = torch.linspace(0, H8 - 1, H8, device=DEV).view(-1, 1).expand(H8, W8).unsqueeze(0)
    img_xy_flatten = torch.cat((img_x, img_y), dim=0).contiguous().view(2, -1)
    pc_features_inline = torch.gather(pc_features, index=lab["pc_kpt_idx"].expand(pc_features.size(0), K), dim=-1)
    pc_xyz_inline = torch.gather(pts.T, index=lab["pc_kpt_idx"].unsqueeze(0).expand(3, K), dim=-1)
    img_inline = torch.gather(img_features, index=lab["coarse_img_kpt_idx"].unsqueeze(0).expand(img_features.size(0), K), dim=-1)
    img_xy_inline = torch.gather(img_xy_flatten, index=lab["coarse_img_kpt_idx"].unsqueeze(0).expand(2, K), dim=-1)
    Pm, K_4 = c["P"][f], c["K_4"][f]
    proj = torch.mm(K_4, (torch.mm(Pm[0:3, 0:3], pc_xyz_inline) + Pm[0:3, 3:]))
    pc_xy = proj[0:2, :] / proj[2:, :]
    mask = (torch.sqrt(torch.sum(torch.square(img_xy_inline.unsqueeze(-1) - pc_xy.unsqueeze(-2)), dim=0)) <= VOpt.dist_thres).float()
    dist64 = 1 - torch.sum(img_inline.double().unsqueeze(-1) * pc_features_inline.double().unsqueeze(-2), dim=0)
    s = c["pc_score"].reshape(-1, N4)[f]
    s_in, s_out = s[lab["pc_kpt_idx"]], s[lab["pc_outline_idx"]]
    stats = torch.stack([s_in.max(), s_in.min(), torch.mean(s_in), s_out.max(), s_out.min(), torch.mean(s_out)])
    return mask, dist64, stats


@pytest.mark.parametrize("idt", [torch.int64, torch.int32])
@pytest.mark.parametrize("B", [1, 6])
@pytest.mark.parametrize("K", [32, 64, 128])
def test_monitors_kernel_against_torch(K, B, idt):
    from cofii2p_amd import ops

    c = _random_case(B, K, seed=100 * K + B, idt=idt)
    assert any(len(torch.unique(c["lab"]["pc_kpt_idx"][f])) < K for f in range(B))
    args = (c["img_desc"], c["pc_desc"], c["W8"], c["points4"], c["pc_score"], c["patches"], c["fine_pc"], c["lab"], c["K_4"], c["P"], VOpt.dist_thres)
    m = ops.val_monitors(*args, topk=5, debug=True)
    torch.cuda.synchronize()
    cnt = torch.full((2,), K, dtype=torch.int32, device=DEV)
    for f in range(B):
        mask, dist64, stats = _torch_expressions(c, f, K)
        # fp32 dot products of 128 unit-vector terms: the bound tests/test_ops_gpu.py puts on row-wise fp32 reductions of this length (1e-6)
        err = float((m["dist"][f].double() - dist64).abs().max())
        print("K %d B %d frame %d: dist err %.3g, n_true %d, counts %s, fine hits %d" % (K, B, f, err, int(m["n_true"][f]), m["counts"][f].tolist(),
                                                                                       int(m["fine_hits"][f])))
        assert err <= 1e-6 + 1e-6 * float(dist64.abs().max())
        assert torch.equal(m["mask"][f], mask)
        row, n = count_by_value(m["dist"][f].cpu(), m["mask"][f].cpu())
        assert int(m["n_true"][f]) == n and n > 0
        assert m["counts"][f].tolist() == row and row[0] > 0 and row[4] > row[0]
        # fine recall: the picks of cofi_fine_match (same cosine, same tie rule) against relative_index (train.py:268-279)
        xy0 = torch.zeros((2, K), device=DEV)
        _fxy, best = ops.fine_match(c["patches"][f].contiguous(), c["fine_pc"][f].contiguous(), xy0, cnt, 1.0)
        rel = c["lab"]["fine_xy"][f].long() - c["lab"]["fine_center_kpt_coors"][f].long() + 2
        hits = int((best.long() == rel[1] * 4 + rel[0]).sum())
        assert int(m["fine_hits"][f]) == hits and hits >= (K + 2) // 3
        assert float((m["score_stats"][f] - stats).abs().max()) <= 1e-6
    # replay of a recording is bit-equal to the eager call
    static = {k: torch.zeros_like(v) for k, v in m.items()}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.val_monitors(*args, topk=5, debug=True, out=static)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        ops.val_monitors(*args, topk=5, debug=True, out=static)
    for v in static.values():
        v.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for k in m:
        assert torch.equal(static[k], m[k]), k


def test_monitors_kernel_limits():
    """(e) beyond what the kernel holds in LDS: COFI_EUNSUPPORTED, no slow path"""
    from cofii2p_amd import _lib, ops

    c = _random_case(1, 32, seed=5)
    K = 129
    lab = {k: torch.zeros((1, K) if v.dim() == 2 else (1, 2, K), dtype=torch.int64, device=DEV) for k, v in c["lab"].items()}
    with pytest.raises(_lib.CofiError, match="COFI_EUNSUPPORTED"):
        ops.val_monitors(c["img_desc"], c["pc_desc"], c["W8"], c["points4"], c["pc_score"], torch.zeros((1, K, 64, 16), device=DEV),
                         torch.zeros((1, K, 64), device=DEV), lab, c["K_4"], c["P"], 1.0)
    wide = torch.zeros((1, 132, 1280), device=DEV), torch.zeros((1, 132, 160), device=DEV)
    with pytest.raises(_lib.CofiError, match="COFI_EUNSUPPORTED"):
        ops.val_monitors(wide[0], wide[1], c["W8"], c["points4"], c["pc_score"], c["patches"], c["fine_pc"], c["lab"], c["K_4"], c["P"], 1.0)
    torch.cuda.synchronize()


@pytest.mark.parametrize("idt", [torch.int64, torch.int32])
@pytest.mark.parametrize("C", [1, 13, 128])
def test_val_gather_against_padded_slices(C, idt):
    """cofi_val_gather on its own: windows that leave the map on every side, centres far outside it (2**40 as int64) and row indices
    outside [0, N1) against zero-padding and slicing on the CPU, exactly; and, as both run one window body, against
    extract_patches_nhwc / gather_rows per frame"""
    from cofii2p_amd import ops

    B, K, H2, W2, N1, PAD = 3, 7, 6, 10, 50, 8
    g = torch.Generator().manual_seed(1000 + C)
    fmap, fpc = torch.randn(B * H2 * W2, C, generator=g), torch.randn(B * N1, C, generator=g)
    far = 2 ** 40 if idt == torch.int64 else 7
    xs, ys, rows = [-1, 0, 1, W2 - 1, W2 + 3, 4, far], [H2 + 3, H2 - 1, 1, 0, -1, 2, 3], [-1, N1, 0, N1 - 1, 17, 3, 42]
    ctr = torch.tensor([[xs[-f:] + xs[:-f], ys[-2 * f:] + ys[:-2 * f]] for f in range(B)])
    if idt == torch.int64:
        ctr[2, 1, ctr[2, 0] == 4] = -far     # ... and in y, on the other side
    idx = torch.tensor([rows[-f:] + rows[:-f] for f in range(B)])
    pat, fp = ops.val_gather(fmap.to(DEV), H2, W2, fpc.to(DEV), ctr.to(idt).to(DEV), idx.to(idt).to(DEV))
    padded = torch.nn.functional.pad(fmap.reshape(B, H2, W2, C), (0, 0, PAD, PAD, PAD, PAD))
    want_pat, want_fp = torch.zeros(B, K, C, 16), torch.zeros(B, K, C)
    for f in range(B):
        for k in range(K):
            x, y, r = int(ctr[f, 0, k]), int(ctr[f, 1, k]), int(idx[f, k])
            if 2 - PAD <= x <= W2 + PAD - 2 and 2 - PAD <= y <= H2 + PAD - 2:
                want_pat[f, k] = padded[f, y - 2 + PAD:y + 2 + PAD, x - 2 + PAD:x + 2 + PAD].permute(2, 0, 1).reshape(C, 16)
            if 0 <= r < N1:
                want_fp[f, k] = fpc[f * N1 + r]
    assert torch.equal(pat.cpu(), want_pat) and torch.equal(fp.cpu(), want_fp)
    assert int((want_pat.abs().sum((2, 3)) == 0).sum()) >= B and int((want_pat != 0).sum()) > 0
    cnt = torch.tensor([K, 0], dtype=torch.int32, device=DEV)
    for f in range(B):
        near = (ctr[f, 0] >= -2) & (ctr[f, 0] < W2 + 2) & (ctr[f, 1] >= -2) & (ctr[f, 1] < H2 + 2)
        xy = torch.where(near, ctr[f], 0).float().to(DEV)
        one = ops.extract_patches_nhwc(fmap[f * H2 * W2:(f + 1) * H2 * W2].to(DEV), H2, W2, xy, cnt, K, 1.0)
        assert int(near.sum()) >= 3 and torch.equal(pat[f][near.to(DEV)], one[near.to(DEV)])
        valid = (idx[f] >= 0) & (idx[f] < N1)
        got = ops.gather_rows(fpc[f * N1:(f + 1) * N1].to(DEV), idx[f][valid].int().to(DEV))
        assert torch.equal(fp[f][valid.to(DEV)], got)


# ------------------------------------------------------------------------------------------ fixture frames
def _fixture_frames(gold, n=6):
    out = []
    for f in range(n):
        fr, data = frame_inputs(int(gold["frame_ids"][f]), int(gold["num_points"]), int(gold["pyr_seed"]))
        assert sha(fr.points) == str(gold["sha_points_%d" % f]) and sha(fr.img) == str(gold["sha_img_%d" % f]) and sha(fr.feats) == str(gold["sha_feats_%d" % f])
        pc = {k: [t.to(DEV) for t in data[k]] for k in ("points", "neighbors", "subsampling", "upsampling")}
        pc["feats"] = data["feats"].to(DEV)
        lab = {k: torch.from_numpy(gold["lab%d_%s" % (f, k)]).to(DEV) for k in ("K_4", "P", "pc_kpt_idx", "pc_outline_idx", "coarse_img_kpt_idx",
                                                                                "fine_center_kpt_coors", "fine_xy", "fine_pc_inline_index")}
        sample = {"img": torch.from_numpy(fr.img).to(DEV), "pc_data_dict": pc}
        sample.update({k: v for k, v in lab.items() if k != "fine_xy"})
        sample["fine_xy_coors"] = lab["fine_xy"]
        out.append((sample, pc, torch.from_numpy(fr.img)[None].to(DEV), lab))
    return out


def test_stack_mode_val_equals_single_frames(model):
    """(b) six frames through ONE mode='val' submission == six forward(mode='val') calls (descriptors and scores to the tolerance
    tests/test_forward_gpu.py::test_stack_mode_batch_equals_single_frames applies, 2e-5); patches / fine_pc bit-equal to a gather from
    that submission's own maps"""
    from cofii2p_amd.network import CoFiI2P
    from cofii2p_amd.validation import stack_labels

    gold = load_golden("val_ref.npz")
    frames = _fixture_frames(gold)
    model.enable_graphs(False)
    model.eval()
    seq = [[t.clone() for t in model(pc, img, lab["fine_center_kpt_coors"], lab["fine_xy"], lab["fine_pc_inline_index"], "val")[:6]]
           for _s, pc, img, lab in frames]
    stacked, imgs = CoFiI2P.stack_frames([f[1] for f in frames], [f[2] for f in frames])
    labels = stack_labels([f[3] for f in frames])
    for idt in (torch.int64, torch.int32):
        handle = model.forward_val_async(4, stacked, imgs, labels["fine_center_kpt_coors"].to(idt), labels["fine_pc_inline_index"].to(idt))
        got = model.finish_val(handle)
        assert len(got) == 6 and got[0][6] is None and got[0][7] is None
        o0 = handle["out"][0]
        B, K = 6, int(gold["num_kpt"])
        C2 = o0["fine_pc_map"].shape[1]
        H2, W2 = Opt.img_H // 2, Opt.img_W // 2
        assert tuple(o0["patches_all"].shape) == (B, K, C2, 16) and tuple(o0["fine_pc_all"].shape) == (B, K, C2)
        fmap = o0["fine_img_map"].reshape(B, H2, W2, C2)
        N1 = o0["fine_pc_map"].shape[0] // B
        for f in range(B):
            for a, b in zip(seq[f][:4], got[f][:4]):
                assert a.shape == b.shape
                d = float((a - b).abs().max())
                assert d < 2e-5, (f, d)
            assert tuple(got[f][4].shape) == (K, C2, 4, 4) and tuple(got[f][5].shape) == (K, C2)
            assert float((seq[f][4] - got[f][4]).abs().max()) < 2e-5 and float((seq[f][5] - got[f][5]).abs().max()) < 2e-5
            ctr = labels["fine_center_kpt_coors"][f]
            want = torch.stack([fmap[f, int(ctr[1, k]) - 2:int(ctr[1, k]) + 2, int(ctr[0, k]) - 2:int(ctr[0, k]) + 2].permute(2, 0, 1) for k in range(K)])
            assert torch.equal(got[f][4], want)
            assert torch.equal(got[f][5], o0["fine_pc_map"][f * N1:(f + 1) * N1][labels["fine_pc_inline_index"][f]])
    # (e) the refusals stay: mode='train' takes one frame, and forward() takes no stack in mode='val'
    with pytest.raises(ValueError):
        model._run_device(None, stacked["points"], stacked["neighbors"], stacked["subsampling"], stacked["upsampling"], stacked["feats"], imgs, "train",
                          labels["fine_center_kpt_coors"], labels["fine_pc_inline_index"])
    with pytest.raises(ValueError):
        model(stacked, imgs, frames[0][3]["fine_center_kpt_coors"], None, frames[0][3]["fine_pc_inline_index"], "val")
    with pytest.raises(ValueError):
        model.forward_async(4, stacked, imgs, mode="val")


def test_validate_reproduces_the_reference_test_acc(model):
    """(c) validate() on the fixture's frames: the reference's counts, n_true, fine hits and acc exactly, score statistics to 1e-5.
    The fixture is well conditioned by construction (tests/tools/make_golden_val.py asserts it in float64): no case is left out."""
    from cofii2p_amd.validation import validate

    gold = load_golden("val_ref.npz")
    frames = _fixture_frames(gold)
    model.enable_graphs(False)
    model.train()   # validate() evaluates in eval() (train.py:37) and hands the module back as it was
    res = validate(model, (f[0] for f in frames), VOpt, slot=3)
    assert model.training
    model.eval()
    print("counts", res["counts"].tolist(), "n_true", res["n_true"].tolist(), "fine_hits", res["fine_hits"].tolist(), "acc", res["acc"].tolist())
    print("score stats err", float((res["score_stats"] - torch.from_numpy(gold["score_stats"])).abs().max()))
    assert torch.equal(res["counts"], torch.from_numpy(gold["counts"]))
    assert torch.equal(res["n_true"], torch.from_numpy(gold["n_true"]))
    assert torch.equal(res["fine_hits"], torch.from_numpy(gold["fine_hits"]))
    assert torch.equal(res["acc"], torch.from_numpy(gold["acc"]))
    assert float((res["score_stats"] - torch.from_numpy(gold["score_stats"])).abs().max()) <= 1e-5
    assert not res["acc"].is_cuda and tuple(res["recall"].shape) == (6, 5)
    # three validation frames: still averaged over the reference's six rows (train.py:31,103)
    res3 = validate(model, [f[0] for f in frames[:3]], VOpt, slot=3)
    assert torch.equal(res3["counts"], torch.from_numpy(gold["counts"][:3])) and torch.equal(res3["acc"], torch.from_numpy(gold["acc3"]))
    # an iterable longer than six frames: the first six are taken (train.py:35-36)
    res8 = validate(model, [f[0] for f in frames] + [frames[0][0], frames[1][0]], VOpt, slot=3)
    assert torch.equal(res8["acc"], torch.from_numpy(gold["acc"]))


def test_validate_groups_frames_of_different_sizes(model):
    """frames of two sizes in one pass: one submission per size on the same slot, rows back in the ORIGINAL frame order, acc divided by the
    LAST frame's n_true.  Each group is the same submission as validate() on that group alone, so the rows must be identical."""
    from cofii2p_amd.preprocess import build_pyramid
    from cofii2p_amd.synth import make_frame, subsample_indices
    from cofii2p_amd.validation import reference_acc, validate

    gold = load_golden("val_ref.npz")
    small = [f[0] for f in _fixture_frames(gold, 4)]
    K, g, big = int(gold["num_kpt"]), torch.Generator().manual_seed(3), []
    for fid in (41, 42):
        fr = make_frame(fid, 4096)
        pyr = build_pyramid(torch.from_numpy(fr.points).to(DEV), [torch.from_numpy(s_).to(DEV) for s_ in subsample_indices(4096, 5, seed=fid)])
        pyr["feats"] = torch.from_numpy(fr.feats).to(DEV)
        N4, N1 = pyr["points"][-1].shape[0], pyr["points"][1].shape[0]
        ctr = torch.stack([torch.randint(2, 254, (K,), generator=g), torch.randint(2, 78, (K,), generator=g)])
        big.append({"img": torch.from_numpy(fr.img).to(DEV), "pc_data_dict": pyr, "K_4": small[0]["K_4"], "P": small[0]["P"],
                    "pc_kpt_idx": torch.randint(0, N4, (K,), generator=g).to(DEV), "pc_outline_idx": torch.randint(0, N4, (K,), generator=g).to(DEV),
                    "coarse_img_kpt_idx": torch.randint(0, 20 * 64, (K,), generator=g).to(DEV), "fine_center_kpt_coors": ctr.to(DEV),
                    "fine_xy_coors": (ctr + torch.randint(-2, 2, (2, K), generator=g)).to(DEV),
                    "fine_pc_inline_index": torch.randint(0, N1, (K,), generator=g).to(DEV)})
    assert big[0]["pc_data_dict"]["points"][0].shape != small[0]["pc_data_dict"]["points"][0].shape
    model.enable_graphs(False)
    model.eval()
    r_small, r_big = validate(model, small, VOpt, slot=2), validate(model, big, VOpt, slot=2)
    order = [("s", 0), ("b", 0), ("s", 1), ("s", 2), ("b", 1), ("s", 3)]
    mixed = validate(model, [(small if w == "s" else big)[i] for w, i in order], VOpt, slot=2)
    for name in ("counts", "n_true", "fine_hits", "score_stats"):
        want = torch.stack([(r_small if w == "s" else r_big)[name][i] for w, i in order])
        assert torch.equal(mixed[name], want), (name, mixed[name], want)
    assert len({tuple(r) for r in mixed["score_stats"].tolist()}) == 6
    assert torch.equal(mixed["acc"], reference_acc(mixed["counts"], mixed["n_true"]))
    assert torch.equal(mixed["acc"], torch.mean(mixed["counts"].float() / int(r_small["n_true"][3]), dim=0))   # the last frame is small[3]


# ------------------------------------------------------------------------------------------ (d) the recorded training step
def test_graphed_train_step_monitors():
    """GraphedTrainStep(monitors=True): losses and updated parameters bit-equal to monitors=False; step.monitors == train_monitors on an
    eager step"""
    from cofii2p_amd.network import CoFiI2P
    from cofii2p_amd.train_step import GraphedTrainStep, step_losses
    from cofii2p_amd.validation import train_monitors

    gold = load_golden("val_ref.npz")
    (_s, pc, img, lab), (_s2, pc2, img2, lab2) = _fixture_frames(gold, 2)
    # index lists WITHOUT duplicates for this test: torch's gather backward adds the gradients of a repeated key point with float atomics,
    # whose order differs from run to run (three or more contributions) - nothing to do with the monitors
    g = torch.Generator().manual_seed(7)
    for l_, p_ in ((lab, pc), (lab2, pc2)):
        K_, N4, N1 = l_["pc_kpt_idx"].numel(), p_["points"][-1].shape[0], p_["points"][1].shape[0]
        perm = torch.randperm(N4, generator=g)
        l_["pc_kpt_idx"], l_["pc_outline_idx"] = perm[:K_].to(DEV), perm[K_:2 * K_].to(DEV)
        l_["coarse_img_kpt_idx"] = torch.randperm(20 * 64, generator=g)[:K_].to(DEV)
        l_["fine_pc_inline_index"] = torch.randperm(N1, generator=g)[:K_].to(DEV)
    sd0 = {k: v.clone() for k, v in CoFiI2P(Opt(), arithmetic="bf16x6").state_dict().items()}

    def run(monitors):
        m = CoFiI2P(Opt(), arithmetic="bf16x6").to(DEV)
        m.load_state_dict(sd0)
        opt = torch.optim.Adam(filter(lambda p: p.requires_grad, m.parameters()), lr=torch.full((), 1e-3, device=DEV), capturable=True)
        step = GraphedTrainStep(m, opt, VOpt, monitors=monitors) if monitors is not None else GraphedTrainStep(m, opt, VOpt)
        losses, mons = [], []
        for it in range(4):
            p_, i_, l_ = (pc, img, lab) if it % 2 == 0 else (pc2, img2, lab2)
            if monitors:
                states.append({k: v.detach().clone() for k, v in m.state_dict().items()})   # the weights step `it` starts from
            losses.append(step(p_, i_, l_).cpu().clone())
            mons.append(None if not monitors else {k: v.cpu().clone() for k, v in step.monitors.items()})
        assert step.replays == 3
        return torch.stack(losses), {k: v.detach().clone() for k, v in m.state_dict().items()}, mons, step

    states = []
    l_off, p_off, _m, s_off = run(None)
    l_on, p_on, mons, s_on = run(True)
    assert s_off.monitors is None and not s_off.with_monitors
    assert torch.equal(l_off, l_on), (l_off, l_on)
    diff = [k for k in p_off if not torch.equal(p_off[k], p_on[k])]
    assert not diff, (len(diff), diff[:5])
    # step.monitors of EVERY step - 0 the eager warm-up call, 1 the recording call, 2 and 3 replays - == train_monitors on an eager forward of
    # a fresh module holding the weights that step started from
    K = int(gold["num_kpt"])
    for it in range(4):
        p_, i_, l_ = (pc, img, lab) if it % 2 == 0 else (pc2, img2, lab2)
        m = CoFiI2P(Opt(), arithmetic="bf16x6").to(DEV)
        m.load_state_dict(states[it])
        m.train()
        outs, _mask, _l = step_losses(m, p_, i_, l_, VOpt)
        dbg = train_monitors(outs, p_, l_, VOpt, debug=True)
        print("step %d: counts %s n_true %d fine_hits %d; replay %s" % (it, dbg["counts"].tolist(), int(dbg["n_true"]), int(dbg["fine_hits"]),
                                                                       {k: v.tolist() for k, v in mons[it].items() if k != "score_stats"}))
        for k in ("counts", "n_true", "fine_hits"):
            assert torch.equal(dbg[k].cpu(), mons[it][k]), (it, k, dbg[k], mons[it][k])
        assert float((dbg["score_stats"].cpu() - mons[it]["score_stats"]).abs().max()) <= 1e-6, it
        assert tuple(dbg["counts"].shape) == (1, 5) and 0 <= int(dbg["fine_hits"]) <= K
        assert torch.equal(dbg["mask"][0], _mask)   # the mask behind n_true is the step's own correspondence mask
        del outs, _l
    assert len({tuple(mm["score_stats"].reshape(-1).tolist()) for mm in mons}) == 4   # every step's own values
