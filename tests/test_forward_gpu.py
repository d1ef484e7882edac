"""End-to-end parity of CoFiI2P.forward on the GPU against (i) the reference's recorded outputs
(tests/golden/frame_*.npz) and (ii) the CPU oracle's intermediate taps.  Tolerance: 1e-3 absolute on
L2-normalised descriptors / sigmoid scores (BASELINE.json north_star), exact on integer outputs."""
import contextlib
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import cofi_oracle as O  # noqa: E402
from common import (assert_coarse_mismatches_are_ties, assert_fine_mismatches_are_ties, check_input_hashes, frame_inputs, load_golden,  # noqa: E402
                    synth_sd)

DEV = "cuda:0"
TOL = 1e-3


class Opt:
    img_H, img_W, img_fine_resolution_scale, norm = 160, 512, 32, "gn"


@pytest.fixture(scope="module")
def model():
    """Tests without an explicit arithmetic run the exact-fp32 GEMMs (tight drift bounds against the fp32 oracle); the library
    default, the 3-term bf16 split with its fused normalising loaders / layer tail, is selected per test (monkeypatch)."""
    from cofii2p_amd import ops
    from cofii2p_amd.network import CoFiI2P

    saved, ops.GEMM_MODE = ops.GEMM_MODE, "f32"
    yield CoFiI2P(Opt()).to(DEV)
    ops.GEMM_MODE = saved


def to_dev(data):
    out = {}
    for k, v in data.items():
        if isinstance(v, list):
            out[k] = [t.to(DEV) if torch.is_tensor(t) else t for t in v]
        else:
            out[k] = v.to(DEV)
    return out


def maxdiff(a, b):
    return float((a.detach().cpu().float() - torch.as_tensor(b).float()).abs().max())


@pytest.mark.parametrize("mode", ["val", "test"])
def test_tiny_frame_vs_reference(model, mode):
    gold = load_golden("frame_tiny.npz")
    fr, data = frame_inputs(int(gold["frame_id"]), int(gold["num_points"]), int(gold["pyr_seed"]))
    check_input_hashes(gold, fr, data)
    img = torch.from_numpy(fr.img)[None].to(DEV)
    taps = {}
    res = model(to_dev(data), img, torch.from_numpy(gold["val_kpt"]).to(DEV), None, torch.from_numpy(gold["val_inl"]).to(DEV), mode, taps=taps)
    # intermediate drift against the oracle (fp32 both sides)
    otaps = {}
    with torch.no_grad():
        O.forward(synth_sd(), data, torch.from_numpy(fr.img)[None], torch.from_numpy(gold["val_kpt"]), torch.from_numpy(gold["val_inl"]), mode, taps=otaps)
    for name in ("encoder1_1", "encoder1_2", "encoder2_1", "encoder3_3", "encoder5_3"):
        d = maxdiff(taps[name], otaps[name])
        scale = float(otaps[name].abs().max())
        assert d <= 2e-4 * max(1.0, scale), (name, d, scale)
    assert maxdiff(taps["tok_img"], otaps["tok_img"]) < 1e-4
    assert maxdiff(taps["tok_pc"], otaps["tok_pc"]) < 1e-4
    names = ("img_desc", "pc_desc", "img_score", "pc_score", "patches", "fine_pc", "center_xy", "coarse_pts")
    for n, t in zip(names, res):
        key = "%s_%s" % (mode, n)
        if t is None:
            assert key not in gold.files
            continue
        assert tuple(t.shape) == gold[key].shape, (key, tuple(t.shape), gold[key].shape)
        assert maxdiff(t, gold[key]) <= TOL, (key, maxdiff(t, gold[key]))


def test_kitti_frame_vs_reference(model):
    gold = load_golden("frame_kitti.npz")
    fr, data = frame_inputs(int(gold["frame_id"]), int(gold["num_points"]), int(gold["pyr_seed"]))
    check_input_hashes(gold, fr, data)
    res = model(to_dev(data), torch.from_numpy(fr.img)[None].to(DEV), None, None, None, "test")
    names = ("img_desc", "pc_desc", "img_score", "pc_score", "patches", "fine_pc", "center_xy", "coarse_pts")
    for n, t in zip(names[:4], res[:4]):
        assert maxdiff(t, gold["test_" + n]) <= TOL, (n, maxdiff(t, gold["test_" + n]))
    # matches: identical selection unless a score sits within 1e-5 of the threshold
    ref_xy, got_xy = gold["test_center_xy"], res[6].cpu().numpy()
    assert got_xy.shape == ref_xy.shape, (got_xy.shape, ref_xy.shape)
    assert np.array_equal(res[7].cpu().numpy(), gold["test_coarse_pts"])
    same = (got_xy == ref_xy).all(0)
    # an argmin may flip only on a near-tie of two pixels: every mismatch is checked for its margin
    assert assert_coarse_mismatches_are_ties(res[0], res[1], model.last_match["sel"].cpu().numpy(), got_xy, ref_xy) > 0.9
    assert maxdiff(res[5], gold["test_fine_pc"]) <= TOL
    assert float(np.abs(res[4].cpu().numpy()[same] - gold["test_patches"][same]).max()) <= TOL
    # fine matching in the caller (eval_all.py:99-105) through the HIP kernel vs the oracle
    from cofii2p_amd.network import fine_matching

    fxy, best = fine_matching(res[4], res[5], res[6])
    oxy, obest = O.fine_match(res[4].cpu(), res[5].cpu(), res[6].cpu())
    assert assert_fine_mismatches_are_ties(res[4], res[5], best, obest) > 0.9
    assert np.array_equal(fxy.cpu().numpy()[:, (best.cpu() == obest).numpy()], oxy.numpy()[:, (best.cpu() == obest).numpy()])


def test_gpu_pyramid_bit_exact_and_int64_contract(model):
    """KNN pyramid built by the HIP kernel == tie-defined C oracle; forward accepts int64 tables."""
    from cofii2p_amd.preprocess import build_pyramid
    from cofii2p_amd.synth import make_frame, subsample_indices

    fr = make_frame(5, 4096)
    sub = subsample_indices(4096, 5, seed=3)
    pyr = build_pyramid(torch.from_numpy(fr.points).to(DEV), [torch.from_numpy(s).to(DEV) for s in sub], int64=True)
    import knn_c

    pts = [fr.points]
    for s in sub:
        pts.append(pts[-1][s])
    for i in range(5):
        assert np.array_equal(pyr["neighbors"][i].cpu().numpy(), knn_c.knn(pts[i], pts[i], 128))
        if i < 4:
            assert np.array_equal(pyr["subsampling"][i].cpu().numpy(), knn_c.knn(pts[i], pts[i + 1], 128))
            assert np.array_equal(pyr["upsampling"][i].cpu().numpy(), knn_c.knn(pts[i + 1], pts[i], 128))
    pyr["feats"] = torch.from_numpy(fr.feats).to(DEV)
    out = model(pyr, torch.from_numpy(fr.img)[None].to(DEV), None, None, None, "test")
    assert out[4].shape[0] >= 4 and out[4].shape[1:] == (64, 16)


def test_nearest_only_upsampling_tables_are_exact(model):
    """build_pyramid(upsample_k=1): the (N, 1) up-sampling tables derived from the points' own neighbour rows equal column 0 of the
    SEARCHED tables bit for bit - a lattice cloud full of exact distance ties and duplicates (sub-sampling with replacement), a KITTI-shaped
    pyramid, and a degenerate selection where no neighbour of most points was selected (full scan) - and the forward's outputs do not
    change by a bit."""
    from cofii2p_amd import ops
    from cofii2p_amd.preprocess import build_pyramid
    from cofii2p_amd.synth import make_frame, subsample_indices

    g = np.random.default_rng(8)
    lattice = (g.integers(0, 12, (3000, 3)) * 0.1).astype(np.float32)          # many coincident points, many equal distances
    for pts_np, subs in ((lattice, subsample_indices(3000, 3, seed=1)), (make_frame(5, 4096).points, subsample_indices(4096, 5, seed=3))):
        pts = torch.from_numpy(pts_np).to(DEV)
        sub = [torch.from_numpy(s_).to(DEV) for s_ in subs]
        full = build_pyramid(pts, sub)
        near = build_pyramid(pts, sub, upsample_k=1)
        for a, b in zip(full["upsampling"], near["upsampling"]):
            assert b.shape == (a.shape[0], 1) and torch.equal(a[:, :1], b)
        for k_ in ("neighbors", "subsampling"):
            assert all(torch.equal(a, b) for a, b in zip(full[k_], near[k_]))
    # degenerate: stage 1 = 64 copies of ONE far corner point -> almost no row of neighbors[0] holds a selected point
    far = torch.from_numpy(np.concatenate([g.random((1500, 3)).astype(np.float32), np.full((1, 3), 50.0, np.float32)])).to(DEV)
    sel = torch.full((64,), 1500, dtype=torch.int32, device=DEV)
    nb = ops.knn(far, far, 128)
    got = ops.knn_up_nearest(far, nb, sel)
    want = ops.knn(far[sel.long()].contiguous(), far, 64)[:, :1]
    assert torch.equal(got, want) and int(got.max()) == 0
    # the forward reads column 0 only (functional.py:20): identical outputs
    fr = make_frame(5, 4096)
    sub = [torch.from_numpy(s_).to(DEV) for s_ in subsample_indices(4096, 5, seed=3)]
    img = torch.from_numpy(fr.img)[None].to(DEV)
    outs = []
    model.enable_graphs(False)
    for kk in (None, 1):
        pyr = build_pyramid(torch.from_numpy(fr.points).to(DEV), sub, upsample_k=kk)
        pyr["feats"] = torch.from_numpy(fr.feats).to(DEV)
        outs.append([t.clone() for t in model(pyr, img, None, None, None, "test")])
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_shim_replays_graphs_unasked_and_results_are_owned(monkeypatch):
    """`from model.network import CoFiI2P` (the unchanged caller's class): hipGraph replay without enable_graphs - the first frame's
    results are the caller's own tensors (the second forward does not touch them), equal to the eager launches bit for bit; the set of
    kept input signatures is bounded."""
    from model.network import CoFiI2P as Shim

    from cofii2p_amd.preprocess import build_pyramid
    from cofii2p_amd.synth import make_frame, subsample_indices

    def inputs(fid, n):
        fr = make_frame(fid, n)
        sub = [torch.from_numpy(s_).to(DEV) for s_ in subsample_indices(n, 5, seed=fid)]
        pyr = build_pyramid(torch.from_numpy(fr.points).to(DEV), sub, int64=True)
        pyr["feats"] = torch.from_numpy(fr.feats).to(DEV)
        return pyr, torch.from_numpy(fr.img)[None].to(DEV)

    m = Shim(Opt()).to(DEV)
    a_in, b_in = inputs(21, 4096), inputs(22, 4096)
    with torch.no_grad():
        a = m(a_in[0], a_in[1], None, None, None, "test")
        keep = [t.clone() for t in a]
        lm = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in m.last_match.items()}
        m(b_in[0], b_in[1], None, None, None, "test")            # same signature: the same graph replays over the same static buffers
        assert len(m._graphs) == 1
        for x, y in zip(a, keep):
            assert torch.equal(x, y)
        m.enable_graphs(False)
        e = m(a_in[0], a_in[1], None, None, None, "test")
        for x, y in zip(e, keep):
            assert torch.equal(x, y)
        assert torch.equal(m.last_match["fine_xy"], lm["fine_xy"])
        # mode='val' (train.py's validation pass: int64 label tensors on the device) through the unasked graph == eager launches
        kpt = torch.tensor([[8, 40, 100, 250], [4, 30, 60, 70]], dtype=torch.int64, device=DEV)
        inl = torch.tensor([0, 5, 77, 2000], dtype=torch.int64, device=DEV)
        mv = Shim(Opt()).to(DEV)
        gv = mv(a_in[0], a_in[1], kpt, None, inl, "val")
        assert len(mv._graphs) == 1
        mv.enable_graphs(False)
        for x, y in zip(gv[:6], mv(a_in[0], a_in[1], kpt, None, inl, "val")[:6]):
            assert torch.equal(x, y)
        m2 = Shim(Opt()).to(DEV)
        for i, n in enumerate(range(2048, 2048 + 64 * (m2.MAX_COPY_GRAPHS + 3), 64)):   # a caller whose clouds keep changing size
            p_, i_ = inputs(30 + i, n)
            m2(p_, i_, None, None, None, "test")
        assert len(m2._graphs) == m2.MAX_COPY_GRAPHS


def test_product_refuses_cpu_tensors(model):
    from cofii2p_amd._lib import CofiError

    with pytest.raises(CofiError):
        model({"points": [], "neighbors": [], "subsampling": [], "upsampling": [], "feats": torch.zeros(1, 4)}, torch.zeros(1, 3, 160, 512),
              None, None, None, "test")


def test_hipgraph_replay_equals_eager(model):
    """the captured graph replays the same kernels on the same data; also on a second frame that reuses the
    captured graph.  Every kernel is a fixed-order reduction (no vendor library, no float atomics): replay == eager bit for bit."""
    from cofii2p_amd.preprocess import build_pyramid
    from cofii2p_amd.synth import make_frame, subsample_indices

    outs = {}
    for fid in (11, 12):
        fr = make_frame(fid, 4096)
        sub = [torch.from_numpy(s).to(DEV) for s in subsample_indices(4096, 5, seed=fid)]
        pyr = build_pyramid(torch.from_numpy(fr.points).to(DEV), sub)
        pyr["feats"] = torch.from_numpy(fr.feats).to(DEV)
        img = torch.from_numpy(fr.img)[None].to(DEV)
        model.enable_graphs(False)
        eager = [t.clone() for t in model(pyr, img, None, None, None, "test")]
        efx = model.last_match["fine_xy"].clone()
        model.enable_graphs(True)
        graph = [t.clone() for t in model(pyr, img, None, None, None, "test")]
        gfx = model.last_match["fine_xy"].clone()
        for a, b in zip(eager[:6], graph[:6]):
            assert torch.equal(a, b)
        assert eager[6].shape == graph[6].shape and torch.equal(eager[6], graph[6])   # same kernels, same data: bit-reproducible
        assert efx.shape == gfx.shape
        outs[fid] = graph
    assert len(model._graphs) == 1  # one capture served both frames
    assert not torch.equal(outs[11][1], outs[12][1])
    model.enable_graphs(False)


@pytest.mark.parametrize("switch", ["DECODER_CONCAT", "COFI_KPCONV_RECORDS"])
def test_flipped_switch_records_anew(model, switch):
    """A switch flipped inside the process (network.routing_state is part of every recording's key) is a new recording with the bits
    of the eager launches under that switch; flipped back, the first recording replays again.  DECODER_CONCAT changes the last bits (a
    stale replay shows in the values), COFI_KPCONV_RECORDS=0 gives the same bits (it shows only in the count)."""
    from cofii2p_amd import kpfpn
    from cofii2p_amd.preprocess import build_pyramid
    from cofii2p_amd.synth import make_frame, subsample_indices

    @contextlib.contextmanager
    def flipped():
        with pytest.MonkeyPatch.context() as mp:
            if switch == "DECODER_CONCAT":
                mp.setattr(kpfpn, "DECODER_CONCAT", True)
            else:
                mp.setenv("COFI_KPCONV_RECORDS", "0")
            yield

    fr = make_frame(11, 4096)
    sub = [torch.from_numpy(s).to(DEV) for s in subsample_indices(4096, 5, seed=11)]
    pyr = build_pyramid(torch.from_numpy(fr.points).to(DEV), sub)
    pyr["feats"] = torch.from_numpy(fr.feats).to(DEV)
    img = torch.from_numpy(fr.img)[None].to(DEV)
    run = lambda: [t.clone() for t in model(pyr, img, None, None, None, "test")[:6]]
    model.enable_graphs(False)   # (drops every recording: the eager references come first)
    with flipped():
        eager = run()
    try:
        model.enable_graphs(True)
        first = run()
        n0 = len(model._graphs)
        with flipped():
            second = run()
            assert len(model._graphs) == n0 + 1
        for a, b in zip(second, eager):
            assert torch.equal(a, b)
        if switch == "DECODER_CONCAT":
            assert not all(torch.equal(a, b) for a, b in zip(second, first))
        third = run()
        assert len(model._graphs) == n0 + 1
        for a, b in zip(third, first):
            assert torch.equal(a, b)
    finally:
        model.enable_graphs(False)


def test_forward_async_reads_stable_inputs_in_place(model):
    """forward_async(inputs_stable=True): no staging copy - the graph reads the caller's tensors, one graph per (slot, input set);
    same bits as the staged path; new CONTENT in the same buffers is picked up by the replay; a new buffer set is a new graph."""
    from cofii2p_amd.preprocess import build_pyramid
    from cofii2p_amd.synth import make_frame, subsample_indices

    def inputs(fid):
        fr = make_frame(fid, 4096)
        sub = [torch.from_numpy(s).to(DEV) for s in subsample_indices(4096, 5, seed=fid)]
        pyr = build_pyramid(torch.from_numpy(fr.points).to(DEV), sub)
        pyr["feats"] = torch.from_numpy(fr.feats).to(DEV)
        return pyr, torch.from_numpy(fr.img)[None].to(DEV)

    pa, ia = inputs(41)
    pb, ib = inputs(42)
    staged_a = [t.clone() for t in model.finish(model.forward_async(20, pa, ia))[:6]]
    staged_b = [t.clone() for t in model.finish(model.forward_async(20, pb, ib))[:6]]
    n0 = len(model._graphs)
    place_a = [t.clone() for t in model.finish(model.forward_async(21, pa, ia, inputs_stable=True))[:6]]
    assert len(model._graphs) == n0 + 1
    for x, y in zip(staged_a, place_a):
        assert torch.equal(x, y)
    # same buffers, new content (what a loader recycling its buffers does): the replay reads it
    for k in ("points", "neighbors", "subsampling", "upsampling"):
        for dst, src in zip(pa[k], pb[k]):
            dst.copy_(src)
    pa["feats"].copy_(pb["feats"])
    ia.copy_(ib)
    again = [t.clone() for t in model.finish(model.forward_async(21, pa, ia, inputs_stable=True))[:6]]
    assert len(model._graphs) == n0 + 1
    for x, y in zip(staged_b, again):
        assert torch.equal(x, y)
    # another buffer set on the same slot: its own graph
    model.finish(model.forward_async(21, pb, ib, inputs_stable=True))
    assert len(model._graphs) == n0 + 2
    from cofii2p_amd._lib import CofiError

    bad = dict(pb)
    bad["feats"] = torch.zeros((pb["feats"].shape[0], 8), device=DEV)[:, :4]   # a strided view: would be copied, i.e. not stable
    with pytest.raises(CofiError):
        model.forward_async(21, bad, ib, inputs_stable=True)
    bad = dict(pb)
    bad["neighbors"] = [t.long() for t in pb["neighbors"]]                       # int64 tables are converted, i.e. not read in place
    with pytest.raises(CofiError):
        model.forward_async(21, bad, ib, inputs_stable=True)


def test_frames_in_flight_match_sequential(model):
    """three frames pipelined over two slots/streams give the same results as one-at-a-time forwards"""
    from cofii2p_amd.preprocess import build_pyramid
    from cofii2p_amd.synth import make_frame, subsample_indices

    frames = []
    for fid in (21, 22, 23):
        fr = make_frame(fid, 4096)
        sub = [torch.from_numpy(s).to(DEV) for s in subsample_indices(4096, 5, seed=fid)]
        pyr = build_pyramid(torch.from_numpy(fr.points).to(DEV), sub)
        pyr["feats"] = torch.from_numpy(fr.feats).to(DEV)
        frames.append((pyr, torch.from_numpy(fr.img)[None].to(DEV)))
    model.enable_graphs(False)
    seq = [[t.clone() for t in model(p, i, None, None, None, "test")] for p, i in frames]
    streams = [torch.cuda.Stream(device=DEV) for _ in range(2)]
    handles, got = [None, None], []
    for k, (p, i) in enumerate(frames):
        sl = k % 2
        if handles[sl] is not None:
            got.append([t.clone() for t in model.finish(handles[sl])])
        with torch.cuda.stream(streams[sl]):
            handles[sl] = model.forward_async(sl, p, i)
    order = [0, 1, 2]
    got.append([t.clone() for t in model.finish(handles[1])])  # frame 1
    got.append([t.clone() for t in model.finish(handles[0])])  # frame 2
    for k in order:
        for a, b in zip(seq[k][:4], got[k][:4]):
            assert maxdiff(a, b.cpu()) < 2e-5
        assert seq[k][6].shape == got[k][6].shape
        assert torch.equal(seq[k][7], got[k][7])


def test_kitti_frame_bf16x3_gemms_within_tolerance(model, monkeypatch):
    """the same golden comparison with every dense contraction on the 3-term bf16 split (fp32 accumulate)"""
    from cofii2p_amd import ops

    monkeypatch.setattr(ops, "GEMM_MODE", "bf16x3")
    model.enable_graphs(False)
    gold = load_golden("frame_kitti.npz")
    fr, data = frame_inputs(int(gold["frame_id"]), int(gold["num_points"]), int(gold["pyr_seed"]))
    res = model(to_dev(data), torch.from_numpy(fr.img)[None].to(DEV), None, None, None, "test")
    names = ("img_desc", "pc_desc", "img_score", "pc_score")
    worst = {n: maxdiff(t, gold["test_" + n]) for n, t in zip(names, res[:4])}
    print("bf16x3 max abs diff vs reference:", worst)
    for n, d in worst.items():
        assert d <= TOL, (n, d)
    assert abs(res[6].shape[1] - gold["test_center_xy"].shape[1]) <= 3  # a score may cross the 0.9 threshold


def test_kitti_frame_bf16x6_is_fp32_grade(model, monkeypatch):
    """"bf16x6" (three bf16 planes per operand, six products): the golden frame as close to the reference as the exact-fp32 arithmetic
    is - the same comparison, each arithmetic's worst output deviation printed side by side - and the same matches selected."""
    from cofii2p_amd import ops

    model.enable_graphs(False)
    gold = load_golden("frame_kitti.npz")
    fr, data = frame_inputs(int(gold["frame_id"]), int(gold["num_points"]), int(gold["pyr_seed"]))
    dd, img = to_dev(data), torch.from_numpy(fr.img)[None].to(DEV)
    names = ("img_desc", "pc_desc", "img_score", "pc_score")
    worst, sel = {}, {}
    for mode in ("f32", "bf16x6", "bf16x3"):
        monkeypatch.setattr(ops, "GEMM_MODE", mode)
        res = model(dd, img, None, None, None, "test")
        worst[mode] = max(maxdiff(t, gold["test_" + n]) for n, t in zip(names, res[:4]))
        sel[mode] = model.last_match["sel"].cpu()
    print("max abs diff vs the reference's outputs:", worst)
    assert worst["bf16x6"] <= max(2.0 * worst["f32"], 2e-6), worst      # fp32-grade: within rounding of the exact-fp32 run
    assert worst["bf16x6"] < 0.5 * worst["bf16x3"], worst               # ... and well below the 3-term split
    assert torch.equal(sel["bf16x6"], sel["f32"])


@pytest.mark.parametrize("norm", ["bn", "ln"])
def test_tiny_frame_other_point_encoder_norms(norm, monkeypatch):
    """opt.norm = 'bn' / 'ln' (get_norm(), modules.py:51-60) against the reference built with that option: BatchNorm (running
    statistics) folded into the weights with LeakyReLU / residual in the GEMM epilogue, LayerNorm as the fused row kernel.  Default
    arithmetic (bf16x3), one frame eager + graph replay + a stacked pair."""
    from cofii2p_amd import ops
    from cofii2p_amd.network import CoFiI2P

    monkeypatch.setattr(ops, "GEMM_MODE", "bf16x3")

    class O2(Opt):
        pass

    O2.norm = norm
    m = CoFiI2P(O2()).to(DEV)
    assert ("pc_encoder.encoder1_1.norm.running_mean" in m.state_dict()) == (norm == "bn")
    gold = load_golden("frame_tiny_%s.npz" % norm)
    fr, data = frame_inputs(int(gold["frame_id"]), int(gold["num_points"]), int(gold["pyr_seed"]))
    dd, img = to_dev(data), torch.from_numpy(fr.img)[None].to(DEV)
    taps = {}
    res = m(dd, img, None, None, None, "test", taps=taps)
    for k in gold.files:
        if k.startswith("tap_encoder"):
            v = taps[k[4:]]
            d = maxdiff(v[:: max(1, v.shape[0] // 8)][:8], gold[k])
            assert d <= 5e-4 * max(1.0, float(np.abs(gold[k]).max())), (k, d)
    for n, t in zip(("img_desc", "pc_desc", "img_score", "pc_score"), res[:4]):
        assert maxdiff(t, gold["test_" + n]) <= TOL, (n, maxdiff(t, gold["test_" + n]))
    assert abs(res[6].shape[1] - gold["test_center_xy"].shape[1]) <= 2
    ref = [t.clone() for t in res[:4]]
    m.enable_graphs(True)
    for a, b in zip(ref, m(dd, img, None, None, None, "test")[:4]):
        assert torch.equal(a, b)
    stacked, imgs = CoFiI2P.stack_frames([dd, dd], [img, img])
    for out in m.finish(m.forward_async(3, stacked, imgs)):
        for a, b in zip(ref, out[:4]):
            assert maxdiff(a.cpu(), b.cpu()) < 1e-4   # other GEMM plans for the stacked shapes: another bf16x3 summation order
    if norm == "bn":
        m.train()
        with pytest.raises(NotImplementedError):
            m(dd, img, None, None, None, "test")


def test_kitti_frame_fused_kpconv_optin(model, monkeypatch):
    """COFI_KPCONV_FUSED=1 (narrow KPConv layers as one kernel, cofi_kpconv_fused): same golden comparison, one frame and a stacked
    pair; the layers really take the fused path."""
    from cofii2p_amd import kpfpn, ops
    from cofii2p_amd.network import CoFiI2P

    monkeypatch.setattr(ops, "GEMM_MODE", "bf16x3")
    monkeypatch.setattr(kpfpn, "FUSED_KPCONV", True)
    calls = []
    real = ops.kpconv_fused
    monkeypatch.setattr(ops, "kpconv_fused", lambda *a, **k: (calls.append(a[0].shape), real(*a, **k))[1])
    model.enable_graphs(False)
    gold = load_golden("frame_kitti.npz")
    fr, data = frame_inputs(int(gold["frame_id"]), int(gold["num_points"]), int(gold["pyr_seed"]))
    dd, img = to_dev(data), torch.from_numpy(fr.img)[None].to(DEV)
    res = model(dd, img, None, None, None, "test")
    assert len(calls) == 5, calls   # encoder1_2, 2_1 (32 channels), 2_2, 2_3, 3_1 (64 channels)
    for n, t in zip(("img_desc", "pc_desc", "img_score", "pc_score"), res[:4]):
        assert maxdiff(t, gold["test_" + n]) <= TOL, n
    ref = [t.clone() for t in res[:4]]
    stacked, imgs = CoFiI2P.stack_frames([dd, dd], [img, img])
    for out in model.finish(model.forward_async(6, stacked, imgs)):
        for a, b in zip(ref, out[:4]):
            assert maxdiff(a.cpu(), b.cpu()) < 2e-5


def test_stack_mode_batch_equals_single_frames(model):
    """B = 3 frames stacked through ONE set of launches (per-frame GroupNorm / InstanceNorm / Q-norm statistics,
    frame-local neighbour tables, batched attention) == the same frames run one at a time"""
    from cofii2p_amd.network import CoFiI2P
    from cofii2p_amd.preprocess import build_pyramid
    from cofii2p_amd.synth import make_frame, subsample_indices

    pyrs, imgs = [], []
    for fid in (31, 32, 33):
        fr = make_frame(fid, 4096)
        sub = [torch.from_numpy(s).to(DEV) for s in subsample_indices(4096, 5, seed=fid)]
        pyr = build_pyramid(torch.from_numpy(fr.points).to(DEV), sub)
        pyr["feats"] = torch.from_numpy(fr.feats).to(DEV)
        pyrs.append(pyr)
        imgs.append(torch.from_numpy(fr.img)[None].to(DEV))
    model.enable_graphs(False)
    seq = [[t.clone() for t in model(p, i, None, None, None, "test")] for p, i in zip(pyrs, imgs)]
    stacked, img = CoFiI2P.stack_frames(pyrs, imgs)
    got = model.finish(model.forward_async(5, stacked, img))
    assert len(got) == 3
    for k in range(3):
        for a, b in zip(seq[k][:4], got[k][:4]):
            assert maxdiff(a, b.cpu()) < 2e-5, maxdiff(a, b.cpu())
        assert seq[k][6].shape == got[k][6].shape
        assert torch.equal(seq[k][7], got[k][7])
        # a stacked GEMM may run another tile / split-K plan than the single-frame one: floats agree to rounding, picks up to near-ties
        sel = model.last_match_frames[k]["sel"].cpu().numpy() if hasattr(model, "last_match_frames") else None
        assert assert_coarse_mismatches_are_ties(got[k][0], got[k][1], sel if sel is not None else None, got[k][6].cpu().numpy(),
                                                 seq[k][6].cpu().numpy()) > 0.9


def test_frame_stack_equals_stack_frames(model):
    """preprocess.FrameStack filled frame by frame (one batched copy launch per frame) = CoFiI2P.stack_frames of the same frames, and a
    stack-mode forward reads it in place"""
    from cofii2p_amd.network import CoFiI2P
    from cofii2p_amd.preprocess import FrameStack, build_pyramid
    from cofii2p_amd.synth import make_frame, subsample_indices

    B, pyrs, imgs = 3, [], []
    for b in range(B):
        fr = make_frame(70 + b, 4096)
        sub = [torch.from_numpy(s_).to(DEV) for s_ in subsample_indices(4096, 5, seed=70 + b)]
        pyr = build_pyramid(torch.from_numpy(fr.points).to(DEV), sub)
        pyr["feats"] = torch.from_numpy(fr.feats).to(DEV)
        pyrs.append(pyr); imgs.append(torch.from_numpy(fr.img)[None].to(DEV))
    want, wimg = CoFiI2P.stack_frames(pyrs, imgs)
    stack = FrameStack(pyrs[0], pyrs[0]["feats"], imgs[0], B)
    for rep in range(2):   # the second round hits the cached descriptor tables
        for b in (2, 0, 1):
            stack.put(b, pyrs[b], pyrs[b]["feats"], imgs[b])
    torch.cuda.synchronize()
    for k in ("points", "neighbors", "subsampling", "upsampling"):
        for a, w in zip(stack.pyr[k], want[k]):
            assert torch.equal(a, w), k
    assert torch.equal(stack.pyr["feats"], want["feats"]) and torch.equal(stack.img, wimg)
    model.enable_graphs(True)
    got = model.finish(model.forward_async(11, stack.pyr, stack.img, inputs_stable=True))
    ref = model.finish(model.forward_async(12, want, wimg))
    model.enable_graphs(False)
    for b in range(B):
        for i in range(8):
            assert torch.equal(got[b][i], ref[b][i]), (b, i)


def test_frame_batcher_single_frame_api(model):
    """serving.FrameBatcher: frames go in one at a time, run as stack-mode submissions of `batch` frames (a partly filled stack is padded
    by its last frame), every ticket returns its own frame's 8-tuple = the stack-mode forward of the same frames; a ticket whose stack
    has been reused is refused"""
    from cofii2p_amd.network import CoFiI2P
    from cofii2p_amd.preprocess import build_pyramid
    from cofii2p_amd.serving import FrameBatcher
    from cofii2p_amd.synth import make_frame, subsample_indices

    frames = []
    for b in range(5):
        fr = make_frame(80 + b, 4096)
        sub = [torch.from_numpy(s_).to(DEV) for s_ in subsample_indices(4096, 5, seed=80 + b)]
        pyr = build_pyramid(torch.from_numpy(fr.points).to(DEV), sub, int64=(b % 2 == 1))   # int64 tables (the reference's) are accepted too
        pyr["feats"] = torch.from_numpy(fr.feats).to(DEV)
        frames.append((pyr, torch.from_numpy(fr.img)[None].to(DEV)))
    model.enable_graphs(True)
    fb = FrameBatcher(model, batch=2, streams=2, ring=2, slot_base=20)
    tickets = [fb.submit(p, im) for p, im in frames]         # 2 + 2 + 1 frames: the third stack is flushed by result()
    got = {}
    for i in (4, 2, 3):                                      # stack 0's second round (frame 4, padded) and stack 1
        got[i] = [t.clone() for t in fb.result(tickets[i])]
    with pytest.raises(RuntimeError):
        fb.result(tickets[0])                                # stack 0 was reused for frame 4
    assert fb.submissions == 3
    for pair in ((2, 3), (4, 4)):
        pyrs = [{k: ([CoFiI2P._as_idx32(t) for t in frames[i][0][k]] if k != "points" else frames[i][0][k]) for k in ("points", "neighbors", "subsampling", "upsampling")} for i in pair]
        for i, p in zip(pair, pyrs):
            p["feats"] = frames[i][0]["feats"]
        st, im = CoFiI2P.stack_frames(pyrs, [frames[i][1] for i in pair])
        ref = model.finish(model.forward_async(28, st, im))
        for pos, i in enumerate(pair[:1] if pair[0] == pair[1] else pair):
            for a, b in zip(got[i], ref[pos]):
                assert torch.equal(a, b), (i,)
    model.enable_graphs(False)


def test_frame_batcher_one_bad_frame_does_not_wedge_the_ring(model, monkeypatch):
    """a frame with fewer than 4 coarse matches at every threshold (CoFiI2P._slice_result raises for it) fails ITS ticket only: the other
    frame of the stack is served, the handle is cleared, and the stack is reused by later submissions"""
    from cofii2p_amd.preprocess import build_pyramid
    from cofii2p_amd.serving import FrameBatcher
    from cofii2p_amd.synth import make_frame, subsample_indices

    frames = []
    for b in range(4):
        fr = make_frame(90 + b, 4096)
        sub = [torch.from_numpy(s_).to(DEV) for s_ in subsample_indices(4096, 5, seed=90 + b)]
        pyr = build_pyramid(torch.from_numpy(fr.points).to(DEV), sub, int64=True)
        pyr["feats"] = torch.from_numpy(fr.feats).to(DEV)
        frames.append((pyr, torch.from_numpy(fr.img)[None].to(DEV)))
    model.enable_graphs(True)
    fb = FrameBatcher(model, batch=2, streams=1, ring=2, slot_base=40)
    real = model._slice_result
    calls = {"n": 0}

    def flaky(o, n, thr_i):
        calls["n"] += 1
        if calls["n"] == 2:                      # the second frame of the first stack
            return real(o, n, -1)                # -> RuntimeError, as for a frame without matches
        return real(o, n, thr_i)

    monkeypatch.setattr(model, "_slice_result", flaky)
    t = [fb.submit(p, im) for p, im in frames]   # two full stacks
    assert len(fb.result(t[0])) == 8
    with pytest.raises(RuntimeError):
        fb.result(t[1])
    assert len(fb.result(t[2])) == 8 and len(fb.result(t[3])) == 8
    t4 = fb.submit(*frames[0])                   # stack 0 again: its handle was cleared, nothing re-raises
    assert len(fb.result(t4)) == 8
    model.enable_graphs(False)


@pytest.mark.parametrize("fid,gemm", [(41, "bf16x3"), (42, "f32")])
def test_other_kitti_frames_vs_oracle(model, monkeypatch, fid, gemm):
    """KITTI-shaped frames the golden files do not hold, in both arithmetics, through the hipGraph path with two frames in
    flight semantics (forward_async), against the CPU oracle (itself pinned to the reference's outputs)"""
    from cofii2p_amd import ops
    from cofii2p_amd.preprocess import build_pyramid
    from cofii2p_amd.synth import make_frame, subsample_indices

    monkeypatch.setattr(ops, "GEMM_MODE", gemm)
    model.enable_graphs(True)
    fr = make_frame(fid, 20480)
    sub = [torch.from_numpy(s).to(DEV) for s in subsample_indices(20480, 5, seed=fid)]
    pyr = build_pyramid(torch.from_numpy(fr.points).to(DEV), sub)      # bit-exact against the tie-defined KNN oracle (own test)
    pyr["feats"] = torch.from_numpy(fr.feats).to(DEV)
    img = torch.from_numpy(fr.img)[None].to(DEV)
    res = model.finish(model.forward_async(7, pyr, img))
    model.enable_graphs(False)
    data = {k: [t.cpu().long() if t.dtype == torch.int32 else t.cpu() for t in pyr[k]] for k in ("points", "neighbors", "subsampling", "upsampling")}
    data["feats"] = torch.from_numpy(fr.feats)
    with torch.no_grad():
        ref = O.forward(synth_sd(), data, torch.from_numpy(fr.img)[None], None, None, "test")
    for i, n in enumerate(("img_desc", "pc_desc", "img_score", "pc_score")):
        assert maxdiff(res[i], ref[i]) <= TOL, (n, maxdiff(res[i], ref[i]))
    assert abs(res[6].shape[1] - ref[6].shape[1]) <= 3
    if res[7].shape == ref[7].shape:
        assert torch.equal(res[7].cpu(), ref[7])


def _oracle_frame(pyr, fr):
    data = {k: [t.cpu().long() if t.dtype == torch.int32 else t.cpu() for t in pyr[k]] for k in ("points", "neighbors", "subsampling", "upsampling")}
    data["feats"] = torch.from_numpy(fr.feats)
    with torch.no_grad():
        return O.forward(synth_sd(), data, torch.from_numpy(fr.img)[None], None, None, "test")


@pytest.mark.parametrize("gemm", ["bf16x6", "bf16x3"])
def test_batch16_kitti_vs_oracle(model, monkeypatch, gemm):
    """BASELINE configs[2] = the bench's headline submission: 16 KITTI-shaped frames (20 480 points each) stacked through ONE set of
    launches, in the fp32-grade arithmetic the reference-named class ships (bf16x6) and in the 3-term split (normalising loaders, fused
    layer-tail chain, partial-slot attention) - three of the sixteen frames
    against the CPU oracle: descriptors / scores within 1e-3, the matched super-point set exact (up to a score within 1e-5 of
    the 0.9 threshold), coarse pixels equal up to near-ties."""
    from cofii2p_amd import ops
    from cofii2p_amd.network import CoFiI2P
    from cofii2p_amd.preprocess import build_pyramid
    from cofii2p_amd.synth import make_frame, subsample_indices

    monkeypatch.setattr(ops, "GEMM_MODE", gemm)
    B = 16
    frs, pyrs, imgs = [], [], []
    for b in range(B):
        fr = make_frame(100 + b, 20480)
        sub = [torch.from_numpy(s_).to(DEV) for s_ in subsample_indices(20480, 5, seed=100 + b)]
        pyr = build_pyramid(torch.from_numpy(fr.points).to(DEV), sub)
        pyr["feats"] = torch.from_numpy(fr.feats).to(DEV)
        frs.append(fr); pyrs.append(pyr); imgs.append(torch.from_numpy(fr.img)[None].to(DEV))
    model.enable_graphs(True)
    stacked, img = CoFiI2P.stack_frames(pyrs, imgs)
    got = model.finish(model.forward_async(9, stacked, img))
    sels = [m["sel"].cpu().numpy() for m in model.last_match_frames]
    model.enable_graphs(False)
    assert len(got) == B
    for b in (0, 7, 15):
        ref = _oracle_frame(pyrs[b], frs[b])
        for i, n in enumerate(("img_desc", "pc_desc", "img_score", "pc_score")):
            assert maxdiff(got[b][i], ref[i]) <= TOL, (b, n, maxdiff(got[b][i], ref[i]))
        score = ref[3].reshape(-1).numpy()
        near_thr = np.abs(score - np.float32(0.9)) < 1e-5
        if not near_thr.any():
            assert got[b][7].shape == ref[7].shape and torch.equal(got[b][7].cpu(), ref[7]), b   # same super-points, same order
            assert assert_coarse_mismatches_are_ties(got[b][0], got[b][1], sels[b], got[b][6].cpu().numpy(), ref[6].numpy()) > 0.9


@pytest.mark.parametrize("gemm", ["bf16x6", "bf16x3"])
def test_stress_frame_vs_oracle(model, monkeypatch, gemm):
    """BASELINE configs[4]: 896 x 1600 image (22 400 image tokens: 900 is not divisible by 32), 40 960 points,
    the whole forward + matching in the default arithmetic against the CPU oracle (attention evaluated in query chunks there:
    the reference itself would materialise an 8 GB score tensor per call)."""
    from cofii2p_amd import ops
    from cofii2p_amd.network import CoFiI2P
    from cofii2p_amd.preprocess import build_pyramid
    from cofii2p_amd.synth import make_frame, subsample_indices

    class OptS:
        img_H, img_W, img_fine_resolution_scale, norm = 896, 1600, 32, "gn"

    monkeypatch.setattr(ops, "GEMM_MODE", gemm)
    big = CoFiI2P(OptS()).to(DEV)
    fr = make_frame(55, 40960, img_hw=(896, 1600))
    sub = [torch.from_numpy(s_).to(DEV) for s_ in subsample_indices(40960, 5, seed=55)]
    pyr = build_pyramid(torch.from_numpy(fr.points).to(DEV), sub)
    pyr["feats"] = torch.from_numpy(fr.feats).to(DEV)
    res = big(pyr, torch.from_numpy(fr.img)[None].to(DEV), None, None, None, "test")
    assert res[0].shape == (1, 128, 112, 200) and res[1].shape == (128, 2560)
    ref = _oracle_frame(pyr, fr)
    for i, n in enumerate(("img_desc", "pc_desc", "img_score", "pc_score")):
        assert maxdiff(res[i], ref[i]) <= TOL, (n, maxdiff(res[i], ref[i]))
    score = ref[3].reshape(-1).numpy()
    if not (np.abs(score - np.float32(0.9)) < 1e-5).any():
        assert res[7].shape == ref[7].shape and torch.equal(res[7].cpu(), ref[7])
        assert assert_coarse_mismatches_are_ties(res[0], res[1], big.last_match["sel"].cpu().numpy(), res[6].cpu().numpy(), ref[6].numpy()) > 0.9
    del big


def test_eval_all_shaped_caller(model, tmp_path, monkeypatch):
    """The loop body of evaluation/eval_all.py:63-131 with the reference's own statements, the model imported through the
    reference's import path (`from model.network import CoFiI2P`): CPU int64 pc_data_dict moved tensor by tensor with .cuda(),
    forward('test') under torch.no_grad(), the caller-side fine matching written with torch ops, pose (cofi_pnp_ransac in place of
    cv2.solvePnPRansac, absent here), get_P_diff, the per-frame result file.  The HIP fine matching must agree with the caller's
    torch expression, the result file must round-trip through the offline metrics."""
    from model.network import CoFiI2P as ShimCoFiI2P   # the shim package at the repository root

    from cofii2p_amd import metrics, ops
    from cofii2p_amd.network import CoFiI2P, fine_matching
    from cofii2p_amd.pose import get_P_diff, pose_matrix, solve_pnp_ransac

    # the reference-named class IS the implementation with the fp32-grade contractions (bf16x6) as its default: what an unchanged caller gets
    assert issubclass(ShimCoFiI2P, CoFiI2P) and ShimCoFiI2P(Opt()).arithmetic == "bf16x6"
    monkeypatch.setattr(ops, "GEMM_MODE", "bf16x3")   # the process default must not leak into the strict shim
    gold = load_golden("frame_kitti.npz")
    fr, data = frame_inputs(int(gold["frame_id"]), int(gold["num_points"]), int(gold["pyr_seed"]))
    batched = {k: [t[None] for t in data[k]] for k in ("points", "neighbors", "subsampling", "upsampling")}   # DataLoader adds a batch axis of 1
    batched["feats"] = data["feats"][None]
    data = {"img": torch.from_numpy(fr.img)[None], "pc_data_dict": batched,
            "K": torch.tensor([[[300.0, 0, 256.0], [0, 300.0, 80.0], [0, 0, 1.0]]]), "P": torch.eye(4)[None]}   # DataLoader batch of 1
    net = ShimCoFiI2P(Opt())
    net.load_state_dict({k: v.clone() for k, v in synth_sd().items()})   # eval_all.py:49 (strict)
    net = net.cuda()
    with torch.no_grad():
        net.eval()
        img = data["img"].cuda()
        pc_data_dict = data["pc_data_dict"]
        for key in ("points", "neighbors", "subsampling", "upsampling"):
            for j in range(len(pc_data_dict[key])):
                pc_data_dict[key][j] = torch.squeeze(pc_data_dict[key][j]).cuda()
        pc_data_dict["feats"] = torch.squeeze(pc_data_dict["feats"]).cuda()
        assert pc_data_dict["neighbors"][0].dtype == torch.int64
        K = torch.squeeze(data["K"].cuda())
        P = torch.squeeze(data["P"]).cpu().numpy()
        (img_features, pc_features, coarse_img_score, coarse_pc_score, fine_img_feature_patch, fine_pc_inline_feature, fine_center_xy,
         coarse_pc_points) = net(pc_data_dict, img, None, None, None, "test")
        # eval_all.py:98-105, verbatim semantics
        fpf = fine_pc_inline_feature.unsqueeze(-1)
        dist = torch.cosine_similarity(fine_img_feature_patch.unsqueeze(-1), fpf.unsqueeze(-2))
        dist = torch.squeeze(dist)
        predict_index = torch.argmax(dist, dim=1)
        fine_xy = fine_center_xy - 2
        fine_xy[0] = fine_xy[0] + predict_index // 4
        fine_xy[1] = fine_xy[1] + predict_index % 4
    hxy, hidx = fine_matching(fine_img_feature_patch, fine_pc_inline_feature, fine_center_xy)
    assert assert_fine_mismatches_are_ties(fine_img_feature_patch, fine_pc_inline_feature, hidx, predict_index) > 0.9
    agree = (hidx == predict_index).cpu().numpy()
    assert np.array_equal(hxy.cpu().numpy()[:, agree], fine_xy.cpu().numpy()[:, agree])
    res, R, t, inl = solve_pnp_ransac(coarse_pc_points.contiguous(), fine_xy.t().contiguous(), K, iterations=2000)
    assert int(res[0]) in (0, 1)
    T_pred = pose_matrix(R, t)
    t_diff, angles_diff = get_P_diff(T_pred, P) if int(res[0]) else (float("nan"), float("nan"))
    path = metrics.save_frame_result(str(tmp_path), 0, metrics.frame_result(P, T_pred, K, pc_data_dict["points"][1], pc_data_dict["points"][-1],
                                                                             coarse_pc_score, fine_xy, coarse_pc_points))
    back = metrics.load_frame_result(path)
    assert set(back) == set(metrics.FRAME_KEYS) and back["fine_xy"].shape == fine_xy.shape
    assert fine_xy.shape[1] == coarse_pc_points.shape[0] >= 4
    # mode='train' with autograd enabled hands back tensors with a graph (train.py:224-226 + loss.backward() at :285; tests/test_train_gpu.py)
    tr = net(pc_data_dict, img, torch.full((2, 4), 8, device=DEV), None, torch.zeros(4, dtype=torch.int64, device=DEV), "train")
    assert tr[0].requires_grad and tr[4].shape == (4, 64, 4, 4) and tr[6] is None


def test_bench_two_ranks_share_device(tmp_path):
    """`python bench.py --gpus 2` started WITHOUT torchrun spawns its two ranks itself, runs them as one process group (gloo here:
    RCCL refuses two ranks on one GPU), gathers the per-frame results and reports n_gpus = 2"""
    import json
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--share-device", "--dist-backend", "gloo", "--steps", "6",
                          "--warmup", "2", "--points", "4096", "--distinct-frames", "4", "--repeats", "2", "--no-cpu-baseline", "--no-kernel-timing",
                          "--no-batch-sweep", "--batch", "2", "--loader-leg"], env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("{")][-1]
    d = json.loads(line)
    assert d["n_gpus"] == 2 and d["ranks"] == 2 and d["gathered_frame_results"] == 8 and d["value"] > 0
    # per-rank rates (a straggler would show), the gather's own time, and the repeats the median was taken over
    assert len(d["per_rank_frames_per_s"]) == 2 and all(v > 0 for v in d["per_rank_frames_per_s"]) and d["result_gather_ms"] >= 0
    assert d["repeats"] == 2 and len(d["seconds_per_repeat"]) == 2 and d["dtype"] == os.environ.get("COFI_GEMM", "bf16x6") and d["frames_per_step"] == 2
    assert abs(d["value"] - 2 * 12 / max(12 / v for v in d["per_rank_frames_per_s"])) / d["value"] < 0.02
    # the ranks the process group reports, with the device each sits on (the driver's scaling run reads this)
    assert d["rccl"]["ranks"] == 2 and len(d["rccl"]["rank_devices"]) == 2 and sorted(r[2] for r in d["rccl"]["rank_devices"]) == [0, 1]
    # ... and the loader leg on EVERY rank next to the other one's: two FrameLoader worker pools + forwards in one process group
    assert len(d["loader_leg"]["per_rank_frames_per_s"]) == 2 and all(v > 0 for v in d["loader_leg"]["per_rank_frames_per_s"])
