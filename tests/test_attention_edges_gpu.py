"""Softmax attention (csrc/attention.hip, attention_x6.inc, attention_parts.h) and the fused LoFTR layer tail (csrc/transformer_tail.hip)
on the GPU against the float64 restatements of tests/attention_refs.py, at the shapes where tiles, masks, key ranges and frame boundaries
go wrong.  Attention: every case and input regime of attention_refs.CASES / REGIMES in the three arithmetics under the derived bound
(error_bound: C1 = 2, C2 = 1/8 - fixed by tests/test_attention_refs_cpu.py, where a plain float32 evaluation reaches 0.38 of it and the
emulated split arithmetic 0.28), exact outcomes, the in-kernel Q norm, strided operands, head counts, refusals.  Tail: the project's own
tolerances for this kernel (test_loftr_tail_fused_successors: 2e-4 for bf16x3, 2e-5 for bf16x6, 1e-4 on the partials) against float64.

Measured on an MI355X (256 compute units; the cases run KS = 1 .. 8), largest kernel error / bound per arithmetic and regime:
                     flat   peaked  sentinel_up  sentinel_down  v_1e4  v_1e-4
    bf16x6           0.30   0.28    0.20         0.22           0.29   0.30     (presplit: the same bits)
    f32              0.31   0.28    0.26         0.33           0.38   0.30
A build whose tail mask keeps key S (">" for ">=" in mask_tail, then written out in both kernels) fails 399 of the 480 tests of this file."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

import attention_refs as R  # noqa: E402

DEV = "cuda:0"
IDS = [R.case_id(c) for c in R.CASES]


def G(t):
    return None if t is None else t.to(DEV)


def _lib():
    from cofii2p_amd import _lib as L_

    return L_


@pytest.fixture(scope="module")
def ops():
    from cofii2p_amd import ops as _ops

    assert torch.cuda.is_available()
    return _ops


@pytest.fixture(params=["bf16x6", "bf16x6-presplit", "f32"])
def attn(request, ops):
    """`ops` with the attention kernel pinned to one arithmetic (as the fixture of tests/test_ops_gpu.py): the bf16 split with K / V split by
    every workgroup, or once by cofi_attention_kv_planes ("presplit"), or the exact fp32 matrix instruction"""
    old, old_rows = ops.ATTN_MODE, ops.ATTN_PRESPLIT_ROWS
    ops.ATTN_MODE = request.param.split("-")[0]
    ops.ATTN_PRESPLIT_ROWS = 1 if request.param.endswith("presplit") else 0
    yield ops
    ops.ATTN_MODE, ops.ATTN_PRESPLIT_ROWS = old, old_rows


def arith_name(ops):
    return ops.ATTN_MODE + ("-presplit" if ops.ATTN_MODE == "bf16x6" and ops.ATTN_PRESPLIT_ROWS == 1 else "")


def num_cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def run_case(ops, case, inp, **kw):
    frames, L, S, H = case
    return ops.attention(G(inp["q"]), G(inp["k"]), G(inp["v"]), q_colscale=G(inp["cs"]), nhead=H, frames=frames, **kw)


def ratio_to_bound(out, ref64, bound):
    return float(((out.detach().cpu().double() - ref64).abs() / bound).max())


# ------------------------------------------------------------------------------------------------ the key split the device runs
def test_cases_run_the_key_splits_they_were_chosen_for():
    lib = _lib().load()
    n = num_cus()
    lays = {c: R.key_layout(c[1], c[2], c[3], c[0], n) for c in R.CASES}
    ran = sorted({lay["KS"] for lay in lays.values()})
    print("device with %d compute units; KS values the cases run: %s" % (n, ran))
    for (frames, L, S, H), lay in lays.items():   # the restatement is the library's layout: the slot table has frames * H * QB * KS slots
        assert lib.cofi_attention_workspace(L, S, H, 32, frames) == frames * H * lay["QB"] * lay["KS"] * 1088 * 4, (frames, L, S, H)
    if n == 256:
        for c, lay in lays.items():
            assert lay["KS"] == R.EXPECTED_KS[c], (c, lay)
        assert ran == list(range(1, 9))
        assert lays[(16, 128, 70, 4)]["light"] == 1 and lays[(1, 65, 129, 4)]["light"] == 0 and lays[(1, 65, 129, 4)]["QB"] % 2 == 1
    else:
        print("not a 256-CU part: only the coverage of KS in {1, 2, 4, 8} is asserted")
        assert {1, 2, 4, 8} <= set(ran)


# ------------------------------------------------------------------------------------------------ 1. every case, regime, arithmetic
@pytest.mark.parametrize("regime", R.REGIMES)
@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_attention_within_the_bound_of_float64(attn, case, regime):
    """stack-mode cases: every frame against its own keys (attention_refs.reference)"""
    inp = R.case_inputs(case, regime)
    o64, bound = R.reference_and_bound(case, regime)
    out = run_case(attn, case, inp)
    assert tuple(out.shape) == tuple(o64.shape) and bool(torch.isfinite(out).all())
    ratio = ratio_to_bound(out, o64, bound)
    print("RATIO %-15s %-18s %-13s KS %d kernel error / bound = %.4f" % (arith_name(attn), R.case_id(case), regime,
                                                                        R.key_layout(case[1], case[2], case[3], case[0], num_cus())["KS"], ratio))
    assert ratio <= 1.0


# ------------------------------------------------------------------------------------------------ 2. exact outcomes
@pytest.mark.parametrize("case", [c for c in R.CASES if c[2] % 32 and c[0] > 1], ids=R.case_id)
def test_equal_scores_give_the_mean_of_the_frames_own_values(attn, case):
    """k = 0: every key of the frame weighs 1 / S exactly, a key past S or of the next frame shows at once"""
    frames, L, S, H = case
    assert case in [(3, 40, 50, 4), (2, 33, 257, 4), (16, 128, 70, 4)]
    inp = dict(R.case_inputs(case, "flat"))
    inp["k"] = torch.zeros_like(inp["k"])
    out = run_case(attn, case, inp).cpu().double()
    assert bool(torch.isfinite(out).all())
    for f in range(frames):
        q, k, v, cs = R.frame_slices(case, inp, f)
        mean = v.double().mean(0, keepdim=True).expand(L, -1)
        ratio = float(((out[f * L:(f + 1) * L] - mean).abs() / R.error_bound(q, k, v, cs, nhead=H)).max())
        assert ratio <= 1.0, (f, ratio)


@pytest.mark.parametrize("which", ["first", "last"])
def test_key_range_far_below_the_others_stays_finite(attn, which):
    """one key range lowered by 300 in base-2 score: its slot scale 2^(m_s - m) underflows to 0 (and, when it comes first, so does the
    online rescale factor) - the output is finite and that of the other keys"""
    case = R.KS_CASES[4]
    frames, L, S, H = case
    lay = R.key_layout(L, S, H, frames, num_cus())
    kb0, nblk = lay["ranges"][0 if which == "first" else -1] if lay["KS"] > 1 else ((0, lay["P"] // 2) if which == "first" else (lay["P"] // 2, lay["P"] - lay["P"] // 2))
    inp = dict(R.case_inputs(case, "peaked"))
    q, k = inp["q"].clone(), inp["k"].clone() / 8
    lo, hi = kb0 * 32, min((kb0 + nblk) * 32, S)
    for h in range(H):   # channel 0 of every head: 1 in every query, -300 / (log2(e) / sqrt(32)) in the keys of the range, 0 in the others
        q[:, h * 32] = 1.0
        k[:, h * 32] = 0.0
        k[lo:hi, h * 32] = -300.0 * (32 ** 0.5) / R.LOG2E
    inp["q"], inp["k"] = q, k
    out = run_case(attn, case, inp)
    assert bool(torch.isfinite(out).all())
    o64, bound = R.reference(case, inp), R.bound(case, inp)
    ratio = ratio_to_bound(out, o64, bound)
    print("%s: range %s of %d lowered by 300: kernel error / bound = %.4f" % (arith_name(attn), which, lay["KS"], ratio))
    assert ratio <= 1.0
    keep = [s for s in range(S) if not lo <= s < hi]      # the lowered keys weigh nothing: the others' attention, to float64 precision
    rest = R.full_attention(q, k[keep], inp["v"][keep], nhead=H)
    assert float((rest - o64).abs().max()) < 1e-12
    # ... whose bound is the sharp one (the 300 in the scores of the lowered keys makes the bound above loose): in fp32 their weights are 0
    sharp = ratio_to_bound(out, rest, R.error_bound(q, k[keep], inp["v"][keep], nhead=H))
    print("%s: against the bound of the other keys alone: %.4f" % (arith_name(attn), sharp))
    assert sharp <= 1.0


def test_zero_q_column_under_colpart_is_clamped_by_q_eps(attn, monkeypatch):
    """a zero column of Q: the in-kernel fold gives 1 / max(0, q_eps), the column stays 0 - bit-equal to the call with the explicit scale
    (one statistics slab, so both folds are the same sum)"""
    monkeypatch.setattr(attn, "GEMM_MODE", "f32")
    L, S, eps = 40, 50, 1e-6
    g = torch.Generator().manual_seed(4)
    x, w = torch.randn(L, 128, generator=g), torch.randn(128, 128, generator=g) / 11
    w[37] = 0
    k, v = G(torch.randn(S, 128, generator=g)), G(torch.randn(S, 128, generator=g))
    q, part = attn.gemm_colstats(G(x), G(w))
    assert part.shape[0] == 1 and bool((q[:, 37] == 0).all()) and float(part[0, 37, 1]) == 0.0
    cs = attn.col_inv_norm_from_colpart(part, L, 128, eps=eps)
    assert float(cs[37]) == float(torch.tensor(1.0, dtype=torch.float32) / torch.tensor(eps, dtype=torch.float32))
    a = attn.attention(q, k, v, q_colpart=part, q_eps=eps).clone()
    b = attn.attention(q, k, v, q_colscale=cs[None].contiguous())
    assert bool(torch.isfinite(a).all()) and torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ 3. q_colpart
@pytest.mark.parametrize("L", [100, 70])
def test_colpart_equals_col_inv_norm_plus_colscale(attn, monkeypatch, L):
    """one frame, a partial 64-row statistics slab: the partials of gemm_colstats (fp32 arithmetic) folded inside the kernel against
    col_inv_norm + q_colscale, and both against float64"""
    monkeypatch.setattr(attn, "GEMM_MODE", "f32")
    S = 90
    g = torch.Generator().manual_seed(L)
    x, w = G(torch.randn(L, 128, generator=g)), G(torch.randn(128, 128, generator=g) / 11)
    kv = G(torch.randn(S, 256, generator=g))
    q, part = attn.gemm_colstats(x, w)
    assert part.shape[0] == 2
    cs = attn.col_inv_norm(q)
    a = attn.attention(q, kv[:, :128], kv[:, 128:], q_colpart=part).clone()
    b = attn.attention(q, kv[:, :128], kv[:, 128:], q_colscale=cs[None].contiguous()).clone()
    qc, kc, vc, csc = q.cpu(), kv[:, :128].cpu(), kv[:, 128:].cpu(), cs.cpu()
    bound = R.error_bound(qc, kc, vc, csc)
    o64 = R.full_attention(qc, kc, vc, R.col_scale(qc.double()))
    r_ab, r_a, r_b = ratio_to_bound(a, b.cpu().double(), bound), ratio_to_bound(a, o64, bound), ratio_to_bound(b, o64, bound)
    print("%s L %d: |colpart - colscale| / bound = %.4f, colpart %.4f and colscale %.4f of the bound from float64" % (arith_name(attn), L, r_ab, r_a, r_b))
    assert r_ab <= 1.0 and r_a <= 1.0 and r_b <= 1.0
    E = _lib().CofiError
    sentinel = torch.full((L, 128), 7.0, device=DEV)
    with pytest.raises(E):   # a slab table of the wrong height
        attn.attention(q, kv[:, :128], kv[:, 128:], q_colpart=part[:1], out=sentinel)
    with pytest.raises(E):
        attn.attention(q, kv[:, :128], kv[:, 128:], q_colpart=torch.cat([part, part, part[:1]]), out=sentinel)   # 5: neither 64- nor 32-row slabs
    with pytest.raises(E):   # the two forms of the scale are alternatives
        attn.attention(q, kv[:, :128], kv[:, 128:], q_colpart=part, q_colscale=cs[None].contiguous(), out=sentinel)
    torch.cuda.synchronize()
    assert bool((sentinel == 7.0).all())


# ------------------------------------------------------------------------------------------------ 4. strided operands
@pytest.mark.parametrize("case", [(3, 40, 50, 4), (1, 65, 129, 4)], ids=R.case_id)
def test_strided_operands_and_merge_into_a_wide_buffer(attn, case):
    """q / k / v as column slices of (rows, 384) buffers (as the projections leave them), the merge into the right half of a
    (rows, 256) buffer: under the bound, the left half untouched, two calls bit-equal.  In stack mode a frame's K / V end
    (S - 1) * 384 + 32 floats into the buffer - the next frame's rows follow at once"""
    frames, L, S, H = case
    inp = R.case_inputs(case, "flat")
    o64, bound = R.reference_and_bound(case, "flat")
    g = torch.Generator().manual_seed(9)
    qb, kvb = torch.randn(frames * L, 384, generator=g), torch.randn(frames * S, 384, generator=g)
    qb[:, 256:], kvb[:, 128:256], kvb[:, 256:] = inp["q"], inp["k"], inp["v"]
    dq, dkv, dcs = G(qb), G(kvb), G(inp["cs"])
    q, k, v = dq[:, 256:], dkv[:, 128:256], dkv[:, 256:]
    wide = torch.full((frames * L, 256), 7.0, device=DEV)
    parts = attn.attention(q, k, v, q_colscale=dcs, nhead=H, frames=frames, parts=True)
    out = parts.merge(out=wide[:, 128:])
    assert out.data_ptr() == wide[:, 128:].data_ptr() and bool((wide[:, :128] == 7.0).all())
    first = out.clone()
    ratio = ratio_to_bound(first, o64, bound)
    print("%s %s strided: kernel error / bound = %.4f" % (arith_name(attn), R.case_id(case), ratio))
    assert ratio <= 1.0
    again = attn.attention(q, k, v, q_colscale=dcs, nhead=H, frames=frames)
    assert torch.equal(first, again)
    assert torch.equal(first, run_case(attn, case, inp))      # ... and the same bits as from contiguous operands


# ------------------------------------------------------------------------------------------------ 5. head counts and refusals
def test_head_dimension_leading_dimension_and_alignment_are_refused(attn):
    """(nhead = 1, 2, 8 run in test_attention_within_the_bound_of_float64.)  Every refusal returns before any launch: the output keeps
    its sentinel"""
    L_ = _lib()
    lib = L_.load()
    assert lib.cofi_attention_workspace(48, 80, 8, 16, 1) == 0 and lib.cofi_attention_workspace(48, 80, 4, 32, 1) > 0
    g = torch.Generator().manual_seed(2)
    q, k, v = (G(torch.randn(n, 128, generator=g)) for n in (48, 80, 80))
    out = torch.full((48, 128), 7.0, device=DEV)
    with pytest.raises(L_.CofiError):   # 8 heads in 128 columns: head dimension 16
        attn.attention(q, k, v, nhead=8, out=out)
    wide = G(torch.randn(48, 132, generator=g))
    with pytest.raises(L_.CofiError):   # 4 bytes off a 16-byte boundary
        attn.attention(wide[:, 1:129], k, v, out=out)
    kwide = G(torch.randn(80, 132, generator=g))
    with pytest.raises(L_.CofiError):
        attn.attention(q, kwide[:, 1:129], v, out=out)
    # a leading dimension below H * 32: only the C entry points can be asked for one
    ws = torch.empty(lib.cofi_attention_workspace(48, 80, 4, 32, 1), dtype=torch.uint8, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    for fn in (lib.cofi_attention_parts, lib.cofi_attention_parts_bf16x6):
        for ldq, ldk, ldv in ((96, 128, 128), (128, 96, 128), (128, 128, 96)):
            rc = fn(p(q), ldq, p(k), ldk, p(v), ldv, None, None, 0, 0, 1e-12, 48, 80, 4, 32, 32 ** -0.5, 1, p(ws), ws.numel(), None)
            assert rc == L_.COFI_EINVAL
            with pytest.raises(L_.CofiError):
                L_.check(rc, "cofi_attention_parts")
        assert fn(p(q), 128, p(k), 128, p(v), 128, None, None, 0, 0, 1e-12, 48, 80, 8, 16, 16 ** -0.5, 1, p(ws), ws.numel(), None) == L_.COFI_EUNSUPPORTED
    assert lib.cofi_attention_merge(p(ws), ws.numel(), 48, 80, 4, 32, 1, p(out), 96, None) == L_.COFI_EINVAL
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


def test_attention_operand_refusals(ops):
    """Operands that do not fit each other are refused from their metadata, before anything is launched, by the softmax and the linear
    attention alike (ops._attn_operands): the kernels read k and v by the rows of k and nhead heads of HD / nhead columns unchecked"""
    CofiError = _lib().CofiError
    q, k, v = (torch.zeros(n, 128, device=DEV) for n in (40, 50, 50))
    bad = {"k of width 96": dict(k=torch.zeros(50, 96, device=DEV)), "v of shape (49, 128)": dict(v=torch.zeros(49, 128, device=DEV)),
           "nhead = 3": dict(nhead=3), "frames = 3": dict(frames=3), "k on the CPU": dict(k=torch.zeros(50, 128))}
    for fn in (ops.attention_parts, ops.linear_attention):
        for what, change in bad.items():
            kw = dict(q=q, k=k, v=v, nhead=4)
            kw.update(change)
            with pytest.raises(CofiError):
                fn(**kw)
                pytest.fail("%s accepted %s" % (fn.__name__, what))


# ================================================================================================ the fused layer tail
TAIL_MODES = [("bf16x3", 2e-4), ("bf16x6", 2e-5)]


@pytest.fixture(scope="module")
def tail_w():
    """the weights of test_loftr_tail_fused_successors: (reference-named float32 on the CPU, the packed layer on the device)"""
    from cofii2p_amd.transformer import pack_layer

    sd = R.tail_weights()
    return sd, pack_layer({n: G(t) for n, t in sd.items()}, "")


@pytest.fixture(params=[(m, t, f) for m, t in TAIL_MODES for f in (True, False)], ids=lambda p: "%s-%s" % (p[0], "frag" if p[2] else "rows"))
def tail(request, ops, monkeypatch):
    mode, tol, frag = request.param
    monkeypatch.setattr(ops, "GEMM_MODE", mode)
    monkeypatch.setattr(ops, "TAIL_FRAG", frag)
    return ops


def tail_tol(ops):
    return dict(TAIL_MODES)[ops.GEMM_MODE]


def assert_close(got, want, tol, what=""):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    err = (got - want).abs()
    worst = float((err / (tol + tol * want.abs())).max())
    print("%s max |error| %.3g, %.3f of the tolerance %g" % (what, float(err.max()), worst, tol))
    assert worst <= 1.0, what


def rand(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("rows", [1, 31, 32, 33, 95])
def test_tail_strided_x_and_out(tail, tail_w, rows):
    """x = the left half of a (rows, 256) buffer, as the product holds it; out a view into a wider buffer: columns outside stay"""
    sd, w = tail_w
    msg, x = rand(rows, rows, 128), rand(rows + 1000, rows, 128)
    xbuf = torch.full((rows, 256), 5.0, device=DEV)
    xbuf[:, :128] = G(x)
    obuf = torch.full((rows, 200), 7.0, device=DEV)
    out = tail.loftr_tail(G(msg), xbuf[:, :128], w, obuf[:, 8:136])
    assert_close(out, R.layer_tail(msg, x, sd)["out"], tail_tol(tail), "rows %d out:" % rows)
    assert bool((xbuf[:, 128:] == 5.0).all()) and torch.equal(xbuf[:, :128].cpu(), x)
    assert bool((obuf[:, :8] == 7.0).all()) and bool((obuf[:, 136:] == 7.0).all())
    assert torch.equal(out, tail.loftr_tail(G(msg), G(x), w, torch.empty((rows, 128), device=DEV)))   # the same bits from contiguous operands


def q_planes(ops, sd):
    pl = ops.split_planes(G(sd["q_proj.weight"]), ops.tail_planes())
    return ops.fragment_order(pl) if ops.TAIL_FRAG else pl


def test_tail_projection_segment_of_128_columns(tail, tail_w):
    """proj_stage<NPL, 1>: a 128-column segment alone (rows = 33), and as the first of two (128, then 384) with partials (rows = 96);
    y and the partials against float64 of the kernel's own out"""
    sd, w = tail_w
    pw, sfx, tol = q_planes(tail, sd), tail.tail_suffix(), tail_tol(tail)
    wq64 = sd["q_proj.weight"].double()
    wqkv64 = torch.cat([sd["q_proj.weight"], sd["k_proj.weight"], sd["v_proj.weight"]]).double()
    # alone
    rows = 33
    msg, x = G(rand(1, rows, 128)), G(rand(2, rows, 128))
    base = tail.loftr_tail(msg, x, w, torch.empty_like(x))
    ybuf = torch.full((rows, 160), 7.0, device=DEV)
    out = tail.loftr_tail(msg, x, w, torch.empty_like(x), proj=[(pw, ybuf[:, 16:144], None)])
    assert torch.equal(out, base)
    assert_close(ybuf[:, 16:144], out.double().cpu() @ wq64.t(), tol, "128 alone y:")
    assert bool((ybuf[:, :16] == 7.0).all()) and bool((ybuf[:, 144:] == 7.0).all())
    # first of two, with partials on the first
    rows = 96
    msg, x = G(rand(3, rows, 128)), G(rand(4, rows, 128))
    base = tail.loftr_tail(msg, x, w, torch.empty_like(x))
    y0, y1 = torch.empty((rows, 128), device=DEV), torch.empty((rows, 384), device=DEV)
    part0, part1 = torch.empty((3, 128, 2), device=DEV), torch.empty((3, 384, 2), device=DEV)
    out = tail.loftr_tail(msg, x, w, torch.empty_like(x), proj=[(pw, y0, part0), (w["qkv" + sfx], y1, part1)])
    assert torch.equal(out, base)
    o64 = out.double().cpu()
    assert_close(y0, o64 @ wq64.t(), tol, "128 first y:")
    assert_close(y1, o64 @ wqkv64.t(), tol, "384 second y:")
    assert torch.equal(y0, y1[:, :128])                         # the same rows of the same weight in both segments: the same products
    for y, part, name in ((y0, part0, "128"), (y1, part1, "384")):
        want = R.column_partials(y.double().cpu())
        assert_close(part[:, :, 0], want[:, :, 0], 1e-4, name + " partial sums:")
        assert_close(part[:, :, 1], want[:, :, 1], 1e-4, name + " partial squares:")


def test_tail_l2_outputs_with_a_padded_transpose(tail, tail_w):
    """rows = 33: out_l2t is a view with ld_l2t = 40 > rows"""
    sd, w = tail_w
    rows = 33
    msg, x = G(rand(5, rows, 128)), G(rand(6, rows, 128))
    l2 = torch.empty((rows, 128), device=DEV)
    tbuf = torch.full((128, 40), 7.0, device=DEV)
    out = tail.loftr_tail(msg, x, w, torch.empty_like(x), out_l2=l2, out_l2t=tbuf[:, :rows])
    assert torch.equal(out, tail.loftr_tail(msg, x, w, torch.empty_like(x)))
    assert torch.equal(l2, tail.l2norm_rows(out)) and torch.equal(tbuf[:, :rows], l2.t())
    assert bool((tbuf[:, rows:] == 7.0).all())
    assert_close(l2, R.layer_tail(msg.cpu(), x.cpu(), sd)["l2"], tail_tol(tail), "l2:")


PARTS_CASES = [(3, 40, 50, 4), (2, 33, 257, 4), (1, 65, 129, 4)]


@pytest.mark.parametrize("arith", ["f32", "bf16x6"])
@pytest.mark.parametrize("case", PARTS_CASES, ids=R.case_id)
def test_tail_merges_attention_parts_across_frames(tail, tail_w, monkeypatch, case, arith):
    """the message as AttnParts: L % 32 != 0, so a 32-row tile of the tail straddles frames and its loader picks frame and row per row -
    bit-equal to the tail fed the merged matrix, and within the tail's tolerance of the float64 layer tail of the float64 attention"""
    sd, w = tail_w
    frames, L, S, H = case
    monkeypatch.setattr(tail, "ATTN_MODE", arith)
    monkeypatch.setattr(tail, "ATTN_PRESPLIT_ROWS", 0)
    inp = R.case_inputs(case, "flat")
    o64, _ = R.reference_and_bound(case, "flat")
    x = rand(L + S, frames * L, 128)
    parts = run_case(tail, case, inp, parts=True)
    assert isinstance(parts, tail.AttnParts)
    a = tail.loftr_tail(parts, G(x), w, torch.empty((frames * L, 128), device=DEV)).clone()
    b = tail.loftr_tail(parts.merge(), G(x), w, torch.empty((frames * L, 128), device=DEV))
    assert torch.equal(a, b)
    assert_close(a, R.layer_tail(o64, x, sd)["out"], tail_tol(tail), "%s %s:" % (arith, R.case_id(case)))


def layer64(sd, x, src, frames, nhead=4):
    """one LoFTR layer (transformer.py:43-64) per frame in float64"""
    x, src = x.double(), src.double()
    L, S = x.shape[0] // frames, src.shape[0] // frames
    w = {n: t.double() for n, t in sd.items()}
    out = []
    for f in range(frames):
        xf, sf = x[f * L:(f + 1) * L], src[f * S:(f + 1) * S]
        q = xf @ w["q_proj.weight"].t()
        msg = R.full_attention(q, sf @ w["k_proj.weight"].t(), sf @ w["v_proj.weight"].t(), R.col_scale(q), nhead=nhead)
        out.append(R.layer_tail(msg, xf, sd)["out"])
    return torch.cat(out)


@pytest.mark.parametrize("arith", ["f32", "bf16x6"])
def test_layer_with_frames_that_end_inside_a_slab(tail, tail_w, monkeypatch, arith):
    """transformer._layer with frames = 3, L = 40: the projection's statistics slabs straddle frames (explicit per-frame column norms)
    and the fused tail merges the slots of tiles that straddle frames"""
    from cofii2p_amd import transformer

    sd, w = tail_w
    monkeypatch.setattr(tail, "ATTN_MODE", arith)
    frames, L, S = 3, 40, 50
    x, src = rand(11, frames * L, 128), rand(12, frames * S, 128)
    xcat = torch.full((frames * L, 256), 5.0, device=DEV)
    xcat[:, :128] = G(x)
    out = torch.empty((frames * L, 128), device=DEV)
    assert tail.tail_planes() > 0 and frames * L <= transformer.TAIL_MAX_ROWS and L % 64
    transformer._layer(w, xcat, G(src), out, self_attn=False, nhead=4, frames=frames)
    assert_close(out, layer64(sd, x, src, frames), tail_tol(tail), "layer, attention %s:" % arith)
    assert bool((xcat[:, 128:] == 5.0).all())                  # the fused tail keeps LN1's output in LDS


def test_tail_exact_outcomes(tail, tail_w):
    """a zero message row: merged = 0, LN1 = norm1.bias exactly - the row of a tail whose merge weight is 0, whatever its message;
    x = 0 and msg = 0: every row is the same row"""
    from cofii2p_amd.transformer import pack_layer

    sd, w = tail_w
    rows = 70
    msg, x = rand(7, rows, 128), rand(8, rows, 128)
    msg[::2] = 0
    out = tail.loftr_tail(G(msg), G(x), w, torch.empty((rows, 128), device=DEV))
    sd0 = dict(sd)
    sd0["merge.weight"] = torch.zeros(128, 128)
    w0 = pack_layer({n: G(t) for n, t in sd0.items()}, "")
    out0 = tail.loftr_tail(G(rand(9, rows, 128)), G(x), w0, torch.empty((rows, 128), device=DEV))
    assert torch.equal(out[::2], out0[::2]) and not torch.equal(out[1::2], out0[1::2])
    # float64 of the same statement: LN1 = norm1.bias
    m = sd["norm1.bias"].double().expand(rows, -1)
    h = torch.relu(torch.cat([x.double(), m], 1) @ sd["mlp.0.weight"].double().t()) @ sd["mlp.2.weight"].double().t()
    want = x.double() + torch.nn.functional.layer_norm(h, (128,), sd["norm2.weight"].double(), sd["norm2.bias"].double())
    assert_close(out0, want, tail_tol(tail), "merge weight 0:")
    zero = torch.zeros((rows, 128), device=DEV)
    same = tail.loftr_tail(zero, zero, w, torch.empty((rows, 128), device=DEV))
    assert bool(torch.isfinite(same).all()) and bool((same == same[0:1]).all())


def tail_desc(ops, w, msg, x, out):
    """the descriptor ops.loftr_tail fills for a plain message matrix"""
    d = _lib().TailDesc()
    sfx = ops.tail_suffix()
    d.w_frag = 1 if ops.TAIL_FRAG else 0
    d.msg, d.ldm, d.rows, d.frames = msg.data_ptr(), msg.stride(0), msg.shape[0], 1
    d.x, d.ldx, d.planes = x.data_ptr(), x.stride(0), ops.tail_planes()
    d.wm, d.w0, d.w2 = w["merge" + sfx].data_ptr(), w["mlp.0" + sfx].data_ptr(), w["mlp.2" + sfx].data_ptr()
    d.n1_gamma, d.n1_beta, d.n2_gamma, d.n2_beta = (w[n].data_ptr() for n in ("norm1.weight", "norm1.bias", "norm2.weight", "norm2.bias"))
    d.eps, d.out, d.ldo = 1e-5, out.data_ptr(), out.stride(0)
    return d


def test_tail_refusals(tail, tail_w):
    """every refusal of the descriptor is a CofiError and returns before the launch: out keeps its sentinel"""
    L_ = _lib()
    lib = L_.load()
    sd, w = tail_w
    rows = 40
    msg, x = G(rand(1, rows, 128)), G(rand(2, rows, 132))
    out = torch.full((rows, 128), 7.0, device=DEV)
    other = torch.empty((4096,), device=DEV)
    y, part = torch.empty((rows, 384), device=DEV), torch.empty((2, 384, 2), device=DEV)
    l2t = torch.empty((128, rows), device=DEV)
    qkv = w["qkv" + tail.tail_suffix()]

    def seg(d, i):
        d.proj_n[i], d.proj_w[i], d.proj_y[i], d.proj_ldy[i] = 384, qkv.data_ptr(), y.data_ptr(), 384

    def both(d):
        d.parts, d.parts_bytes, d.L, d.S, d.H = other.data_ptr(), other.numel() * 4, rows, 8, 4

    def neither(d):
        d.msg = None

    def second_without_first(d):
        seg(d, 1)

    def partials_on_partial_slab(d):
        seg(d, 0)
        d.proj_part[0] = part.data_ptr()

    def short_l2t(d):
        d.out_l2t, d.ld_l2t = l2t.data_ptr(), rows - 1

    def misaligned_x(d):
        d.x = x.data_ptr() + 4

    def four_planes(d):
        d.planes = 4

    stream = torch.cuda.current_stream().cuda_stream
    for spoil in (both, neither, second_without_first, partials_on_partial_slab, short_l2t, misaligned_x, four_planes):
        d = tail_desc(tail, w, msg, x[:, :128], out)
        spoil(d)
        rc = lib.cofi_loftr_tail(ctypes.byref(d), stream)
        assert rc in (L_.COFI_EINVAL, L_.COFI_EUNSUPPORTED), (spoil.__name__, rc)
        with pytest.raises(L_.CofiError):
            L_.check(rc, "cofi_loftr_tail")
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    # through ops.loftr_tail: a projection's partials need whole 32-row slabs, the planes must be the arithmetic's
    with pytest.raises(L_.CofiError):
        tail.loftr_tail(msg, x[:, :128], w, out, proj=[(qkv, y, part)])
    with pytest.raises(L_.CofiError):
        tail.loftr_tail(msg, x[:, :128], w, out, proj=[(qkv, y, None)] * 3)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    # ... and the unspoilt descriptor runs
    d = tail_desc(tail, w, msg, x[:, :128], out)
    assert lib.cofi_loftr_tail(ctypes.byref(d), stream) == 0
    assert_close(out, R.layer_tail(msg.cpu(), x[:, :128].cpu(), sd)["out"], tail_tol(tail), "descriptor:")
