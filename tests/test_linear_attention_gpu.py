"""Linear attention (attention='linear') on the GPU: the kernels against the float64 restatement (tests/linear_attention_refs.py) under
the derived bound, bit-reproducibility of stacked and repeated calls, one layer and the whole forward against the reference's recorded
outputs (tests/golden/linear_attention_micro.npz, frame_tiny_linear*.npz), the serving paths and the training composition."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import linear_attention_refs as R  # noqa: E402
from common import (assert_coarse_mismatches_are_ties, assert_fine_mismatches_are_ties, check_input_hashes, frame_inputs, load_golden,  # noqa: E402
                    sha)

DEV = "cuda:0"
TOL = 1e-3   # the project's budget on descriptors and scores


class Opt:
    img_H, img_W, img_fine_resolution_scale, norm = 160, 512, 32, "gn"


def G(a):
    return (a if torch.is_tensor(a) else torch.from_numpy(np.asarray(a))).to(DEV)


@pytest.fixture(scope="module")
def ops():
    from cofii2p_amd import ops as _ops

    return _ops


def maxdiff(a, b):
    return float((a.detach().cpu().float() - torch.as_tensor(b).detach().cpu().float()).abs().max())


def bound_ratio(out, q, k, v, cs):
    """largest |out - out64| / bound over the elements (CPU tensors in, float)"""
    o64 = R.linear_attention(q, k, v, cs, dtype=torch.float64)
    return float(((out.detach().cpu().double() - o64).abs() / R.error_bound(q, k, v, cs)).max())


# ------------------------------------------------------------------------------------------------ 1. the kernels
@pytest.mark.parametrize("L,S", R.CASES)
def test_kernel_against_float64_restatement(ops, L, S):
    q, k, v = R.case_inputs(L, S)
    cs = R.col_scale(q)                      # float32: the same scale goes to the kernel and to the restatement
    out = ops.linear_attention(G(q), G(k), G(v), q_colscale=G(cs))
    assert out.shape == (L, 128) and bool(torch.isfinite(out).all())
    ratio = bound_ratio(out, q, k, v, cs)
    print("(%d, %d): kernel error / bound = %.4g" % (L, S, ratio))
    assert ratio <= 1.0


@pytest.mark.parametrize("L,S", [(48, 80), (5, 1), (64, 300)])
def test_all_keys_very_negative_give_exact_zero(ops, L, S):
    """phi(k) underflows to 0: KV = Ksum = 0, Z = 1 / eps, out = 0 - never NaN or Inf"""
    q, _, v = R.case_inputs(L, S)
    out = ops.linear_attention(G(q), torch.full((S, 128), -100.0, device=DEV), G(v), q_colscale=G(R.col_scale(q)))
    assert bool(torch.isfinite(out).all()) and bool((out == 0).all())


def test_strided_operands_stacking_and_repeatability(ops):
    """q / k / v as column slices of (rows, 384) buffers (as the projections leave them), 3 stacked frames, S over two summary chunks
    with a partial tile: every frame bit-equal to its single-frame call, two calls bit-equal, and all of it under the bound"""
    F_, L, S = 3, 70, 300
    g = torch.Generator().manual_seed(5)
    qb, kvb = torch.randn(F_ * L, 384, generator=g) * 0.5, torch.randn(F_ * S, 384, generator=g)
    kvb[:, 128:256] *= 8
    cs = torch.stack([R.col_scale(qb[f * L:(f + 1) * L, :128]) for f in range(F_)])
    dq, dkv, dcs = G(qb), G(kvb), G(cs)
    q, k, v = dq[:, :128], dkv[:, 128:256], dkv[:, 256:]
    wide = torch.zeros((F_ * L, 256), device=DEV)
    out = ops.linear_attention(q, k, v, q_colscale=dcs, frames=F_, out=wide[:, 128:])
    assert out.data_ptr() == wide[:, 128:].data_ptr() and bool((wide[:, :128] == 0).all())
    again = ops.linear_attention(q, k, v, q_colscale=dcs, frames=F_)
    assert torch.equal(out, again)
    for f in range(F_):
        one = ops.linear_attention(q[f * L:(f + 1) * L], k[f * S:(f + 1) * S], v[f * S:(f + 1) * S], q_colscale=dcs[f:f + 1].contiguous())
        assert torch.equal(one, out[f * L:(f + 1) * L]), f
        ratio = bound_ratio(one, qb[f * L:(f + 1) * L, :128], kvb[f * S:(f + 1) * S, 128:256], kvb[f * S:(f + 1) * S, 256:], cs[f])
        assert ratio <= 1.0, (f, ratio)


@pytest.mark.parametrize("frames,L,S", [(1, 130, 80), (2, 128, 65)])
def test_colpart_equals_explicit_colscale(ops, monkeypatch, frames, L, S):
    """q_colpart (the projection GEMM's column partials, folded by cofi_col_inv_norm_from_colpart) against q_colscale from col_inv_norm"""
    monkeypatch.setattr(ops, "GEMM_MODE", "f32")
    g = torch.Generator().manual_seed(L + S)
    x, w = G(torch.randn(frames * L, 128, generator=g)), G(torch.randn(384, 128, generator=g) * 0.1)
    kv = torch.randn(frames * S, 256, generator=g)
    kv[:, :128] *= 8
    dkv = G(kv)
    qkv, part = ops.gemm_colstats(x, w)
    q = qkv[:, :128]
    a = ops.linear_attention(q, dkv[:, :128], dkv[:, 128:], q_colpart=part, frames=frames)
    cs = torch.stack([ops.col_inv_norm(q[f * L:(f + 1) * L]) for f in range(frames)])
    b = ops.linear_attention(q, dkv[:, :128], dkv[:, 128:], q_colscale=cs, frames=frames)
    for f in range(frames):
        sl = slice(f * L, (f + 1) * L)
        bound = R.error_bound(q[sl].cpu(), kv[f * S:(f + 1) * S, :128], kv[f * S:(f + 1) * S, 128:], cs[f].cpu())
        ratio = float(((a[sl] - b[sl]).cpu().double().abs() / bound).max())
        print("frames %d frame %d: |colpart - colscale| / bound = %.4g" % (frames, f, ratio))
        assert ratio <= 1.0
    with pytest.raises(_lib().CofiError):
        ops.linear_attention(q, dkv[:, :128], dkv[:, 128:], q_colpart=part, q_colscale=cs, frames=frames)


def _lib():
    from cofii2p_amd import _lib as L_

    return L_


def test_unsupported_head_dimension_is_refused(ops):
    lib = _lib().load()
    assert lib.cofi_linear_attention_workspace(48, 80, 8, 16, 1) == 0
    assert lib.cofi_linear_attention_workspace(48, 80, 4, 32, 1) > 0
    q, k, v = (G(t) for t in R.case_inputs(48, 80))
    with pytest.raises(_lib().CofiError):
        ops.linear_attention(q, k, v, nhead=8)
    # the C entry point itself refuses before any launch: the output keeps its sentinel
    out = torch.full((48, 128), 7.0, device=DEV)
    ws = torch.empty(1 << 16, dtype=torch.uint8, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = lib.cofi_linear_attention(p(q), 128, p(k), 128, p(v), 128, None, 48, 80, 8, 16, 1e-6, 1, p(out), 128, p(ws), ws.numel(), None)
    torch.cuda.synchronize()
    assert rc == _lib().COFI_EUNSUPPORTED and bool((out == 7.0).all())


# ------------------------------------------------------------------------------------------------ 2. one layer
@pytest.mark.parametrize("arith", ["f32", "bf16x6"])
def test_linear_layer_against_the_reference(ops, monkeypatch, arith):
    from cofii2p_amd.transformer import loftr_layer

    monkeypatch.setattr(ops, "GEMM_MODE", arith)
    mg, lin = load_golden("micro_ops.npz"), load_golden("linear_attention_micro.npz")
    w = {k[len("lay_w_"):]: G(mg[k]) for k in mg.files if k.startswith("lay_w_")}
    out = loftr_layer(w, G(mg["lay_x"]), G(mg["lay_src"]), attention="linear")
    d = maxdiff(out, lin["lay_out"])
    print("%s: max |layer - reference| = %.3g" % (arith, d))
    assert d <= 1e-4
    assert maxdiff(loftr_layer(w, G(mg["lay_x"]), G(mg["lay_src"])), mg["lay_out"]) <= 1e-4   # the default kind is still the softmax layer
    with pytest.raises(ValueError):
        loftr_layer(w, G(mg["lay_x"]), G(mg["lay_src"]), attention="nonsense")


# ------------------------------------------------------------------------------------------------ 3. the whole forward
def to_dev(data):
    return {k: ([t.to(DEV) if torch.is_tensor(t) else t for t in v] if isinstance(v, list) else v.to(DEV)) for k, v in data.items()}


@pytest.fixture(scope="module")
def tiny():
    gold = load_golden("frame_tiny_linear.npz")
    gold_test = load_golden("frame_tiny_linear_test.npz")
    fr, data = frame_inputs(int(gold["frame_id"]), int(gold["num_points"]), int(gold["pyr_seed"]))
    check_input_hashes(gold, fr, data)
    rec = {k: gold[k] for k in gold.files}
    rec.update({k: gold_test[k] for k in gold_test.files})
    return rec, to_dev(data), torch.from_numpy(fr.img)[None].to(DEV)


_MODELS = {}


def linear_model(arith):
    from cofii2p_amd.network import CoFiI2P

    if arith not in _MODELS:
        _MODELS[arith] = CoFiI2P(Opt(), arithmetic=arith, attention="linear").to(DEV)
    return _MODELS[arith]


@pytest.mark.parametrize("mode", ["val", "test"])
@pytest.mark.parametrize("arith", ["f32", "bf16x6"])
def test_tiny_frame_against_the_linear_reference(tiny, arith, mode):
    from cofii2p_amd import transformer
    from cofii2p_amd.network import fine_matching

    gold, data, img = tiny
    assert transformer.FUSED_CHAIN            # the chain switch is on; 'linear' runs layer by layer beside it
    model = linear_model(arith)
    model.enable_graphs(False)
    res = model(data, img, G(gold["val_kpt"]), None, G(gold["val_inl"]), mode)
    for n, t in zip(("img_desc", "pc_desc", "img_score", "pc_score"), res[:4]):
        d = maxdiff(t, gold["%s_%s" % (mode, n)])
        print("%s %s %s: %.3g" % (arith, mode, n, d))
        assert tuple(t.shape) == gold["%s_%s" % (mode, n)].shape and d <= TOL, (n, d)
    if mode == "val":
        assert res[6] is None and res[7] is None
        for n, t in zip(("patches", "fine_pc"), res[4:6]):
            assert maxdiff(t, gold["val_" + n]) <= TOL, n
        return
    # 'test': the selected super-points and their coarse pixels are integer outputs - equal up to near-ties of the similarity
    ref_xy, ref_pts = gold["test_center_xy"], gold["test_coarse_pts"]
    assert tuple(res[6].shape) == ref_xy.shape and tuple(res[7].shape) == ref_pts.shape
    assert maxdiff(res[7], ref_pts) == 0.0                                      # the same super-points passed the score threshold
    sel = model.last_match["sel"].cpu().numpy()
    got_xy = res[6].cpu().numpy()
    same = assert_coarse_mismatches_are_ties(res[0], res[1], sel, got_xy, ref_xy)
    keep = torch.from_numpy((got_xy == ref_xy).all(0))
    assert same > 0.9 and int(keep.sum()) > 0
    assert maxdiff(res[4].cpu()[keep], torch.from_numpy(gold["test_patches"])[keep]) <= TOL
    assert maxdiff(res[5].cpu()[keep], torch.from_numpy(gold["test_fine_pc"])[keep]) <= TOL
    # the fine pick (eval_all.py:99-102) on the reference's recorded patches, in float64, against this implementation's
    p_ref, f_ref = torch.from_numpy(gold["test_patches"])[keep].double(), torch.from_numpy(gold["test_fine_pc"])[keep].double()
    ref_best = torch.nn.functional.cosine_similarity(p_ref, f_ref[:, :, None], dim=1).argmax(1)
    kd = keep.to(DEV)
    _, best = fine_matching(res[4][kd], res[5][kd], res[6][:, kd])
    assert_fine_mismatches_are_ties(res[4][kd], res[5][kd], best, ref_best)


def test_default_kind_is_untouched_by_a_linear_model(tiny):
    """two default models, one built and run before and one after a linear model ran: bit-equal, and not the linear result"""
    from cofii2p_amd.network import CoFiI2P

    gold, data, img = tiny
    a = CoFiI2P(Opt(), arithmetic="f32").to(DEV)
    ra = [t.clone() for t in a(data, img, None, None, None, "test")]
    lin = [t.clone() for t in linear_model("f32")(data, img, None, None, None, "test")]
    b = CoFiI2P(Opt(), arithmetic="f32").to(DEV)
    rb = b(data, img, None, None, None, "test")
    assert a.attention == b.attention == "full"
    for x, y in zip(ra, rb):
        assert x.shape == y.shape and torch.equal(x, y)
    assert not torch.equal(ra[1], lin[1])
    ref = load_golden("frame_tiny.npz")
    assert maxdiff(ra[1], ref["test_pc_desc"]) <= TOL


# ------------------------------------------------------------------------------------------------ 4. serving paths
def _frame(fid):
    from cofii2p_amd.preprocess import build_pyramid
    from cofii2p_amd.synth import make_frame, subsample_indices

    fr = make_frame(fid, 4096)
    sub = [torch.from_numpy(s).to(DEV) for s in subsample_indices(4096, 5, seed=fid)]
    pyr = build_pyramid(torch.from_numpy(fr.points).to(DEV), sub)
    pyr["feats"] = torch.from_numpy(fr.feats).to(DEV)
    return pyr, torch.from_numpy(fr.img)[None].to(DEV)


@pytest.fixture(scope="module")
def frames3():
    return [_frame(f) for f in (31, 32, 33)]


def test_stack_mode_batch_equals_single_frames(frames3):
    from cofii2p_amd.network import CoFiI2P

    model = linear_model("f32")
    model.enable_graphs(False)
    seq = [[t.clone() for t in model(p, i, None, None, None, "test")] for p, i in frames3]
    stacked, img = CoFiI2P.stack_frames([p for p, _ in frames3], [i for _, i in frames3])
    got = model.finish(model.forward_async(5, stacked, img))
    assert len(got) == 3
    for k in range(3):
        for a, b in zip(seq[k][:4], got[k][:4]):
            assert maxdiff(a, b) < 2e-5, (k, maxdiff(a, b))   # (a stacked GEMM may run another plan: rounding, as for the softmax kind)
        assert seq[k][6].shape == got[k][6].shape and torch.equal(seq[k][7], got[k][7])
        sel = model.last_match_frames[k]["sel"].cpu().numpy()
        assert assert_coarse_mismatches_are_ties(got[k][0], got[k][1], sel, got[k][6].cpu().numpy(), seq[k][6].cpu().numpy()) > 0.9


def test_rig_submission_equals_repeated_cloud(frames3):
    from cofii2p_amd.network import CoFiI2P

    model = linear_model("f32")
    cloud, imgs = frames3[0][0], [frames3[1][1], frames3[2][1]]
    rig, img = CoFiI2P.stack_frames([cloud], imgs)
    rep, img_rep = CoFiI2P.stack_frames([cloud, cloud], imgs)
    assert torch.equal(img, img_rep)
    want = [[t.clone() for t in o] for o in model.finish(model.forward_async(7, rep, img))]
    got = model.finish(model.forward_async(8, rig, img, cameras=2))
    assert len(got) == len(want) == 2
    for k in range(2):
        for i, (a, b) in enumerate(zip(want[k][:4], got[k][:4])):
            assert maxdiff(a, b) < 2e-5, (k, i, maxdiff(a, b))
        assert want[k][6].shape == got[k][6].shape and torch.equal(want[k][7], got[k][7])
        sel = model.last_match_frames[k]["sel"].cpu().numpy()
        assert assert_coarse_mismatches_are_ties(got[k][0], got[k][1], sel, got[k][6].cpu().numpy(), want[k][6].cpu().numpy()) > 0.9
    assert not torch.equal(got[0][1], got[1][1])


def test_forward_async_replay_equals_eager(frames3):
    model = linear_model("bf16x6")
    pyr, img = frames3[0]
    model.enable_graphs(False)
    eager = [t.clone() for t in model(pyr, img, None, None, None, "test")]
    first = [t.clone() for t in model.finish(model.forward_async(11, pyr, img))]     # records, then replays
    second = model.finish(model.forward_async(11, pyr, img))                          # replays only
    for a, b, c in zip(eager, first, second):
        assert a.shape == b.shape == c.shape and torch.equal(a, b) and torch.equal(a, c)


# ------------------------------------------------------------------------------------------------ 5. training
LAYER_WEIGHTS = ("q_proj.weight", "k_proj.weight", "v_proj.weight", "merge.weight", "mlp.0.weight", "mlp.2.weight", "norm1.weight", "norm1.bias",
                 "norm2.weight", "norm2.bias")


def test_linear_layer_gradients_are_fp32_grade(ops, monkeypatch):
    """train_forward.loftr_layer(attention='linear') at (L, S) = (48, 80): gradients for x, src and all weights against the float64
    restatement under autograd; gate: at most 2 x the error of the float32 restatement on the CPU against the same float64, floor
    1e-6 * max|grad| per tensor"""
    from cofii2p_amd import train_forward

    monkeypatch.setattr(ops, "GEMM_MODE", "f32")
    mg = load_golden("micro_ops.npz")
    w0 = {n: torch.from_numpy(mg["lay_w_" + n]) for n in LAYER_WEIGHTS}
    x0, s0 = torch.from_numpy(mg["lay_x"]), torch.from_numpy(mg["lay_src"])
    probe = torch.linspace(-1, 1, x0.numel()).reshape(x0.shape)

    def cpu_grads(dtype):
        leaf = lambda t: t.to(dtype).clone().requires_grad_()   # (a copy: .to() of a float32 tensor to float32 is the tensor itself)
        w = {n: leaf(t) for n, t in w0.items()}
        x, s = leaf(x0), leaf(s0)
        out = R.loftr_layer(w, x, s, dtype=dtype)
        (out * probe.to(dtype)).sum().backward()
        return out.detach(), dict({n: t.grad for n, t in w.items()}, x=x.grad, src=s.grad)

    o64, g64 = cpu_grads(torch.float64)
    o32, g32 = cpu_grads(torch.float32)
    P = {"l." + n: G(t).requires_grad_() for n, t in w0.items()}
    x, s = G(x0).requires_grad_(), G(s0).requires_grad_()
    out = train_forward.loftr_layer(P, "l.", x, s, attention="linear")
    (out * G(probe)).sum().backward()
    got = dict({n: P["l." + n].grad for n in LAYER_WEIGHTS}, x=x.grad, src=s.grad)
    e_out, e_out32 = float((out.detach().cpu().double() - o64).abs().max()), float((o32.double() - o64).abs().max())
    print("output: |gpu - f64| %.3g, |cpu32 - f64| %.3g" % (e_out, e_out32))
    assert e_out <= max(2 * e_out32, 1e-6 * float(o64.abs().max()))
    for n, ref in g64.items():
        e, e32 = float((got[n].cpu().double() - ref).abs().max()), float((g32[n].double() - ref).abs().max())
        floor = 1e-6 * float(ref.abs().max())
        print("%-14s |gpu - f64| %.3g   |cpu32 - f64| %.3g   floor %.3g" % (n, e, e32, floor))
        assert e <= max(2 * e32, floor), (n, e, e32, floor)


def test_graphed_train_step_is_bit_identical_to_eager():
    """GraphedTrainStep with attention='linear' on the tiny frame: the recorded-and-replayed step (the second call; the first runs
    eagerly) against the eager step from the same state - losses and every parameter, bit for bit"""
    from cofii2p_amd.network import CoFiI2P
    from cofii2p_amd.train_step import GraphedTrainStep, train_step

    gold = load_golden("train_ref.npz")
    fr, data = frame_inputs(int(gold["frame_id"]), int(gold["num_points"]), int(gold["pyr_seed"]))
    assert sha(fr.points) == str(gold["sha_points"]) and sha(fr.img) == str(gold["sha_img"])
    dd = {k: [t.to(DEV) for t in v] for k, v in data.items() if k in ("points", "neighbors", "subsampling", "upsampling")}
    dd["feats"] = data["feats"].to(DEV)
    img = torch.from_numpy(fr.img)[None].to(DEV)
    batch = {k[4:]: G(gold[k]) for k in gold.files if k.startswith("lab_")}

    class StepOpt:
        dist_thres, pos_margin, neg_margin = float(gold["dist_thres"]), float(gold["pos_margin"]), float(gold["neg_margin"])

    sd0 = {k: v.clone() for k, v in CoFiI2P(Opt(), arithmetic="bf16x6", attention="linear").state_dict().items()}

    def run(graphed):
        m = CoFiI2P(Opt(), arithmetic="bf16x6", attention="linear").to(DEV)
        m.load_state_dict(sd0)
        opt = torch.optim.Adam(filter(lambda p: p.requires_grad, m.parameters()), lr=torch.full((), 1e-3, device=DEV), capturable=True)
        step = GraphedTrainStep(m, opt, StepOpt) if graphed else None
        losses = [(step(dd, img, batch) if graphed else torch.stack(train_step(m, opt, dd, img, batch, StepOpt))).clone() for _ in range(2)]
        if graphed:
            assert step.replays == 1
        return torch.stack(losses).cpu(), {k: v.detach().clone() for k, v in m.state_dict().items()}

    l_e, p_e = run(False)
    l_g, p_g = run(True)
    print("losses eager %s\nlosses graphed %s" % (l_e.tolist(), l_g.tolist()))
    assert bool(torch.isfinite(l_e).all()) and not torch.equal(l_e[0], l_e[1])      # the weights moved between the two steps
    off = {k: int((p_e[k] != p_g[k]).sum()) for k in p_e if not torch.equal(p_e[k], p_g[k])}
    print("parameters that differ: %d tensors, %d elements" % (len(off), sum(off.values())))
    assert torch.equal(l_e, l_g)
    assert not off, off
