"""The backward operators of cofii2p_amd/autograd.py (csrc/backward.hip) at the shapes where their kernels change path: support rows
listed 0, 64, 65, 128 and 200 times (the list walks stage 64 pairs per round), column-block views as operands and as incoming gradients,
attention with fewer keys than one block / one query / one key / large logits / the bf16x6 forward, row-block reductions at every
boundary of `rows_per_block`, arg-max ties in and across lane groups, clamped norms, convolution geometries with untouched pixels, the
grid-stride loop of the up-sampling adjoint.  Every case goes through the public functions of cofii2p_amd.autograd, compares the forward
value and every gradient with float64 torch.autograd (or the hand-written float64 references of tests/backward_refs.py) of the same
operator, and runs forward + backward twice: the gradients must be bit-identical (csrc/backward.hip: fixed summation order).
Needs a real MI355X:  python -m pytest tests/test_backward_edges_gpu.py -m gpu"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import backward_refs as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def G(a, grad=False):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV) if isinstance(a, np.ndarray) else a.to(DEV)
    return t.requires_grad_() if grad else t


def rel_err(a, b):
    b = b.detach().double()
    a = a.detach().double().to(b.device)
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def max_err(a, b):
    """largest deviation relative to the largest reference entry (the measure of test_attention_bf16x6_against_the_fp32_instruction_kernel)"""
    b = b.detach().double()
    a = a.detach().double().to(b.device)
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


@pytest.fixture(autouse=True)
def f32_arithmetic(monkeypatch):
    from cofii2p_amd import ops

    monkeypatch.setattr(ops, "GEMM_MODE", "f32")


def backward_through_cat(y, dy):
    """y.backward(dy) with dy arriving the way the network delivers it: as a column block (offset 4, longer rows) of the gradient of a
    torch.cat([...], 1) - a view that autograd._rows hands to the kernel in place."""
    M, C = y.shape
    W = (C + 4 + 8 + 3) // 4 * 4
    wide = torch.full((M, W), 7.0, device=DEV)     # a kernel that ignores the leading dimension reads these
    wide[:, 4:4 + C] = dy
    seen = []
    y.register_hook(lambda g: seen.append((g.stride(0), g.storage_offset())))
    left, right = (torch.zeros((M, n), device=DEV, requires_grad=True) for n in (4, W - 4 - C))
    torch.cat([left, y, right], 1).backward(wide)
    assert seen == [(W, 4)], "the gradient did not arrive as a column block of the wide buffer"


def send(y, dy, strided):
    backward_through_cat(y, dy) if strided else y.backward(dy)


def same_twice(run):
    """run() -> (forward value, gradients ...): twice from fresh leaves; the gradients must be the same bits"""
    a, b = run(), run()
    for i, (x, y) in enumerate(zip(a[1:], b[1:])):
        assert torch.equal(x, y), "gradient %d differs between two runs" % i
    return a


def assert_rows(got, ref, tol, rows, scale=None):
    """the named rows one by one: ||got[j] - ref[j]|| <= tol ||scale[j]|| (scale = ref unless given), an all-zero reference row exactly"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    scale = ref if scale is None else scale.detach().double().cpu()
    for j in rows:
        if float(scale[j].abs().max()) == 0.0:
            assert float(got[j].abs().max()) == 0.0, j
        else:
            assert float((got[j] - ref[j]).norm()) <= tol * float(scale[j].norm()), (j, float((got[j] - ref[j]).norm() / scale[j].norm()))


# ------------------------------------------------------------------------------------------ 1. KPConv aggregation
KP_COUNTS = [0, 64, 65, 128, 200]


def _kp_case(C):
    from cofii2p_amd.weights import kernel_point_table

    g = np.random.default_rng(100 + C)
    N, M, H, sigma = 300, 180, 24, 0.3
    s_pts = G((g.random((N, 3)) * 0.4).astype(np.float32))
    q_pts = G((g.random((M, 3)) * 0.4).astype(np.float32))
    idx_np = R.fan_in_table(g, N, M, H, KP_COUNTS, repeat=(4, 5))
    idx = G(idx_np.astype(np.int32))
    kp = G(kernel_point_table(15, 0.425 * sigma / 0.2))
    feats = G(g.standard_normal((N, C)).astype(np.float32))
    dagg = G(g.standard_normal((M, 15 * C)).astype(np.float32))
    return N, M, H, sigma, s_pts, q_pts, idx_np, idx, kp, feats, dagg


@pytest.mark.parametrize("C,strided", [(8, False), (32, False), (64, False), (64, True), (96, False), (192, False), (256, False), (256, True)])
def test_kpconv_aggregate_long_and_empty_lists(C, strided):
    """support rows listed 0 / 64 / 65 / 128 / 200 times (one query lists row 4 five times): no round, one full round, a round + 1, two
    full rounds, three rounds + a tail of 8; C = 8: eight pairs side by side, 96: a half-used second chunk, 192 / 256: 3 / 4 chunks"""
    from cofii2p_amd import autograd as ag

    N, M, H, sigma, s_pts, q_pts, idx_np, idx, kp, feats, dagg = _kp_case(C)

    def run():
        f = feats.clone().requires_grad_()
        agg, _ = ag.kpconv_aggregate(f, q_pts, s_pts, idx, kp, sigma, ag.TableCache())
        send(agg, dagg, strided)
        return agg.detach(), f.grad

    agg, df = same_twice(run)
    ragg, rdf, infl = R.kpconv_aggregate_ref(feats, q_pts, s_pts, idx, kp, sigma, dagg)
    live = (infl.sum(-1) > 0).cpu().numpy()
    for j in (1, 2, 3, 4):    # the long lists prove something only if their pairs carry weight
        assert live[idx_np == j].mean() >= 0.5, (j, live[idx_np == j].mean())
    assert rel_err(agg, ragg) < 1e-5
    assert rel_err(df, rdf) < 1e-5
    assert_rows(df, rdf, 1e-5, range(5))
    assert float(df[0].abs().max()) == 0.0        # the empty list still writes its row (df comes from torch.empty)


def test_kpconv_aggregate_refuses_a_narrow_width_that_is_no_power_of_two():
    from cofii2p_amd import _lib, autograd as ag

    N, M, H, sigma, s_pts, q_pts, idx_np, idx, kp, feats, dagg = _kp_case(48)
    f = feats.clone().requires_grad_()
    agg, _ = ag.kpconv_aggregate(f, q_pts, s_pts, idx, kp, sigma, ag.TableCache())
    with pytest.raises(_lib.CofiError):
        agg.backward(dagg)


# ------------------------------------------------------------------------------------------ 2. neighbour max-pool
def _maxpool_case(C, H):
    """-> x (N, C), idx (M, H), dy, and the queries carrying the planted ties.  Lane group of neighbour h in the arg-max kernel: h & 7."""
    g = np.random.default_rng(1000 * H + C)
    N, M = 150, 90
    # 90 H slots: the fan-in of case 1 (0 / 64 / 65 / 200 listings) needs 329 of them; H = 1 has room for 0 / 64 only
    counts = [0, 64, 65, 200] if H >= 7 else [0, 64]
    planted = (20, 21, 22, 23, 24)
    idx = R.fan_in_table(g, N, M, H, counts, repeat=(3, 5) if H >= 7 else None, keep_free_of=planted)
    idx[np.isin(idx, (130, 131, 132, 133, 145))] = 100                   # these rows are listed by the planted queries alone
    x = g.standard_normal((N, C)).astype(np.float32)
    x[130] = x[131] = 8.0 + g.standard_normal(C).astype(np.float32)      # two DIFFERENT rows with equal values, above everything else
    x[132] = x[133] = 9.0 + g.standard_normal(C).astype(np.float32)
    x[140:145] = -0.1 - np.abs(x[140:145])                               # all-negative rows
    x[145] = 0.0                                                         # a real row that equals the pad row
    neg = 140 + np.arange(H) % 5
    for m in planted:
        idx[m] = neg
    ties = {}
    across = (3, 12) if H > 12 else ((3, 5) if H > 5 else None)           # equal maxima in different lane groups
    if across:
        idx[20, across[0]], idx[20, across[1]] = 130, 131
        ties["across"] = (20, 130, 131, across[0])
    within = (2, 10) if H > 10 else ((0, 8) if H > 8 else None)           # equal maxima in the same lane group
    if within:
        idx[21, within[0]], idx[21, within[1]] = 132, 133
        ties["within"] = (21, 132, 133, within[0])
    idx[22, H // 2] = N                                                  # all negative + one pad entry: output 0, no gradient
    if H >= 3:
        idx[23, 1], idx[23, 2] = N, 145                                  # pad first, then a feature of exactly 0.0: the pad wins
        idx[24, 1], idx[24, 2] = 145, N                                  # the other way round: the feature wins
    got = np.bincount(idx.reshape(-1), minlength=N + 1)[:len(counts)]
    assert list(got) == counts
    dy = g.standard_normal((M, C)).astype(np.float32)
    return N, M, G(x), idx, G(idx.astype(np.int32)), G(dy), ties


@pytest.mark.parametrize("H", [1, 7, 9, 37, 256])
@pytest.mark.parametrize("C,strided", [(4, False), (36, True), (96, False), (160, True)])
def test_neighbor_maxpool_first_maximum_row_by_row(C, H, strided):
    from cofii2p_amd import autograd as ag

    N, M, x, idx_np, idx, dy, ties = _maxpool_case(C, H)

    def run():
        x1 = x.clone().requires_grad_()
        y = ag.neighbor_maxpool(x1, idx, ag.TableCache())
        send(y, dy, strided)
        return y.detach(), x1.grad

    y, dx = same_twice(run)
    ry, rdx, arg = R.maxpool_first_max_ref(x, idx, dy)
    _, mag, _ = R.maxpool_first_max_ref(x, idx, dy.abs())     # what each row actually sums, in magnitude: the scale of its rounding error
    assert torch.equal(y.double().cpu(), ry)                  # a maximum of fp32 values is exact
    assert rel_err(dx, rdx) < 1e-6
    assert_rows(dx, rdx, 1e-6, range(N), scale=mag)           # row by row, tied rows NOT folded together
    # the planted cases, spelled out
    dxc, dyc = dx.cpu(), dy.cpu()
    for kind, (m, first, second, h) in ties.items():          # the first of the two equal rows takes the whole gradient, the second nothing
        assert bool((arg[m] == h).all()), kind
        assert torch.equal(dxc[first], dyc[m]) and float(dxc[second].abs().max()) == 0.0, kind
    assert float(y[22].abs().max()) == 0.0
    if H >= 3:
        assert float(y[23].abs().max()) == 0.0 and float(y[24].abs().max()) == 0.0
        assert bool((arg[23] == 1).all()) and bool((arg[24] == 1).all())
        assert torch.equal(dxc[145], dyc[24])                 # listed by queries 23 (behind the pad) and 24 (before it) only
    assert float(dxc[0].abs().max()) == 0.0                   # never listed


def test_neighbor_maxpool_refuses_more_than_256_neighbours():
    from cofii2p_amd import _lib, autograd as ag

    g = np.random.default_rng(0)
    x = G(g.standard_normal((150, 4)).astype(np.float32), grad=True)
    idx = G(g.integers(0, 150, (90, 257)).astype(np.int32))
    with pytest.raises(_lib.CofiError):
        ag.neighbor_maxpool(x, idx, ag.TableCache())


# ------------------------------------------------------------------------------------------ 3. row gather
@pytest.mark.parametrize("C", [4, 64, 65, 130])
@pytest.mark.parametrize("form,strided", [("column", False), ("column", True), ("list", False), ("list", True)])
def test_gather_rows_long_lists(form, C, strided):
    """N = 10 rows gathered 2000 times: about 200 rows per list (the nearest up-sampling's fan-in), support row 0 never; as the first
    column of an (M, H) table and as a 1-D list with repeats"""
    from cofii2p_amd import autograd as ag

    g = np.random.default_rng(C)
    N, M = 10, 2000
    x = G(g.standard_normal((N, C)).astype(np.float32))
    first = g.integers(1, N, M)
    first[::50] = N                                                       # shadow entries: a zero row out, nothing back
    if form == "column":
        idx_np = g.integers(0, N + 1, (M, 3))                             # the other columns are not part of the operator
        idx_np[:, 0] = first
    else:
        idx_np = first
    idx = G(idx_np.astype(np.int32))
    dy = G(g.standard_normal((M, C)).astype(np.float32))

    def run():
        x1 = x.clone().requires_grad_()
        y = ag.gather_rows(x1, idx, ag.TableCache())
        send(y, dy, strided)
        return y.detach(), x1.grad

    y, dx = same_twice(run)
    xr = x.double().clone().requires_grad_()
    yr = torch.cat([xr, torch.zeros((1, C), device=DEV, dtype=torch.float64)], 0)[G(first)]
    yr.backward(dy.double())
    mag = torch.zeros((N + 1, C), device=DEV, dtype=torch.float64).index_add_(0, G(first), dy.double().abs())[:N]
    assert torch.equal(y.double(), yr.detach())
    assert rel_err(dx, xr.grad) < 1e-6
    assert_rows(dx, xr.grad, 1e-6, range(N), scale=mag)
    assert float(dx[0].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------ 4. attention
# The bound test_attention_bf16x6_against_the_fp32_instruction_kernel grants the bf16x6 forward: 5e-6 of the largest output.  It is used
# here, unchanged, for that forward against float64 and for the two gradients that inherit O through delta = dO . O (dQ, dK).
BF16X6_BOUND = 5e-6
ATTN_SHAPES = [(33, 5, 4, 0.7), (1, 1, 4, 0.7), (65, 1, 1, 0.7), (1, 97, 2, 0.7), (97, 129, 8, 0.7), (64, 31, 4, 0.7), (64, 32, 4, 0.7),
               (64, 33, 4, 0.7), (70, 200, 4, 6.0), (70, 200, 4, 12.0)]
_attn_cache = {}


def _attn_case(L, S, H, qs):
    """inputs, the float64 reference and the error of plain fp32 torch autograd against it (computed once per shape, shared by the
    layouts and arithmetics, never changed)"""
    key = (L, S, H, qs)
    if key in _attn_cache:
        return _attn_cache[key]
    D = 32
    g = torch.Generator().manual_seed(1000 * L + S)
    q = torch.randn((L, H * D), generator=g) * qs
    k, v, do = (torch.randn((n, H * D), generator=g) for n in (S, S, L))
    if qs > 1.0:
        # large logits: key block 5 (keys 160 ... 191) belongs to wave 1 and is that wave's second block; it holds every row's maximum, so
        # both rescales of pass 1 - inside a wave and across the waves - carry the result
        k *= 0.15
        k[160:192] *= 1.25 / 0.15
        logit = torch.einsum("lhd,shd->hls", q.double().reshape(L, H, D), k.double().reshape(S, H, D)) / math.sqrt(D)
        assert bool(((logit.argmax(-1) // 32) == 5).all())
        assert float(logit.max()) > (20.0 if qs == 6.0 else 40.0)
    ref = R.attention_ref(q, k, v, do, H)
    r32 = [t.clone().requires_grad_() for t in (q, k, v)]
    A = torch.softmax(torch.einsum("lhd,shd->hls", r32[0].reshape(L, H, D), r32[1].reshape(S, H, D)) / math.sqrt(D), dim=-1)
    o32 = torch.einsum("hls,shd->lhd", A, r32[2].reshape(S, H, D)).reshape(L, H * D)
    o32.backward(do)
    t32 = (o32.detach(), r32[0].grad, r32[1].grad, r32[2].grad)
    err32 = {fn.__name__: [fn(a, b) for a, b in zip(t32, ref)] for fn in (rel_err, max_err)}
    _attn_cache[key] = (q, k, v, do, ref, err32)
    return _attn_cache[key]


@pytest.mark.parametrize("arith", ["f32", "bf16x6"])
@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("L,S,H,qs", ATTN_SHAPES)
def test_attention_edge_shapes(L, S, H, qs, packed, arith):
    """fewer keys than one block (three of the four waves idle), one key, one query, 32 k + 1 sizes, 1 / 2 / 8 heads, logits up to 28 and
    57; contiguous operands and q | k | v (S == L) or k | v as column blocks of one projection buffer; the forward in f32 and in bf16x6
    arithmetic (training's default: O, hence delta, then comes from the split kernel while the backward recomputes P in exact fp32)"""
    from cofii2p_amd import autograd as ag, ops

    HD = H * 32
    q, k, v, do, ref, err32 = _attn_case(L, S, H, qs)
    qg, kg, vg, dog = G(q), G(k), G(v), G(do)

    def run():
        if not packed:
            leaves = [t.clone().requires_grad_() for t in (qg, kg, vg)]
            ins = leaves
        elif S == L:
            leaves = [torch.cat([qg, kg, vg], 1).requires_grad_()]
            ins = leaves[0].split(HD, 1)                      # train_forward.py: q, k, v = qkv.split(C, 1)
        else:
            leaves = [qg.clone().requires_grad_(), torch.cat([kg, vg], 1).requires_grad_()]
            ins = [leaves[0], *leaves[1].split(HD, 1)]
        with ops.arithmetic(arith):
            o = ag.attention(*ins, nhead=H)
        o.backward(dog)
        if not packed:
            grads = [t.grad for t in leaves]
        elif S == L:
            grads = list(leaves[0].grad.split(HD, 1))
        else:
            grads = [leaves[0].grad, *leaves[1].grad.split(HD, 1)]
        return (o.detach(), *[t.contiguous() for t in grads])

    o, dq, dk, dv = same_twice(run)
    # f32: the project's operator tolerances (1e-5 forward, 2e-5 gradients, relative Frobenius error).  Measured on MI355X at q scale
    # 0.7: forward <= 1.9e-7, gradients <= 3.1e-7 (plain fp32 torch: 2.4e-7 / 2.7e-7).
    # bf16x6 forward: BF16X6_BOUND in its own measure for o, dq, dk; dv does not read O and keeps 2e-5.  Measured against float64,
    # of the largest entry: o <= 2.8e-7, dq / dk <= 5.3e-7 at q scale 0.7; o 9.3e-7 / 1.7e-6, dq 1.9e-6 / 4.1e-6 at q scale 6 / 12.
    # Large logits (q scale 6 / 12): the allowance is max(tolerance, 4 x the error of plain fp32 torch autograd against float64 on the same
    # inputs - 1.4e-6 relative, 2.6e-6 of the largest entry at scale 12): two fp32 evaluations of one formula differ by about twice either's error, and the kernel's summation
    # order is not torch's.  Measured, f32: dq 1.6e-6 / 3.0e-6, dk 1.5e-6 / 2.9e-6 at q scale 6 / 12 (fp32 torch: 9.8e-7 / 1.4e-6) -
    # inside the plain tolerance, so the allowance is not drawn on.
    x6 = arith == "bf16x6"
    fwd, fwd_tol = (max_err, BF16X6_BOUND) if x6 else (rel_err, 1e-5)
    grd, grd_tol = (max_err, BF16X6_BOUND) if x6 else (rel_err, 2e-5)
    allow = lambda fn, tol, i: max(tol, 4.0 * err32[fn.__name__][i]) if qs > 1.0 else tol
    print("attention", (L, S, H, qs), "packed" if packed else "contiguous", arith,
          "kernel o dq dk dv: %.2e %.2e %.2e %.2e" % (fwd(o, ref[0]), grd(dq, ref[1]), grd(dk, ref[2]), rel_err(dv, ref[3])),
          "| fp32 torch: %.2e %.2e %.2e %.2e" % (err32[fwd.__name__][0], err32[grd.__name__][1], err32[grd.__name__][2], err32["rel_err"][3]))
    assert fwd(o, ref[0]) < allow(fwd, fwd_tol, 0)
    if S == 1:
        # one key: P == 1, dS = 0, the exact dQ and dK are zero - judged absolutely, against the size of the terms that cancel
        bound = 1e-5 * float(do.abs().max()) * float(v.abs().max()) * float(k.abs().max())
        assert float(dq.abs().max()) < bound and float(dk.abs().max()) < bound
    else:
        assert grd(dq, ref[1]) < allow(grd, grd_tol, 1)
        assert grd(dk, ref[2]) < allow(grd, grd_tol, 2)
    assert rel_err(dv, ref[3]) < allow(rel_err, 2e-5, 3)


# ------------------------------------------------------------------------------------------ 5. GroupNorm + activation
def _gn_reference(x, ga, be, r, groups, slope, fixed, dy, dtype):
    """leaky(group_norm(x) * gamma + beta + res, slope) and its gradients with torch.autograd in `dtype` (on the tensors' device)"""
    ref = [t.to(dtype).clone().requires_grad_() if t is not None else None for t in (x, ga, be, r)]
    if fixed is not None:
        z = (ref[0] - fixed[0].to(dtype)) * torch.rsqrt(fixed[1].to(dtype) + 1e-5)
        if ga is not None:
            z = z * ref[1] + ref[2]
    else:
        z = F.group_norm(ref[0].t().unsqueeze(0), groups, ref[1], ref[2], 1e-5).squeeze(0).t()
    if r is not None:
        z = z + ref[3]
    yr = F.leaky_relu(z, slope) if slope != 1.0 else z
    yr.backward(dy.to(dtype))
    return yr.detach(), [t.grad if t is not None else None for t in ref]


def _gn_run(M, C, groups, affine, slope, res, fixed, strided, mean=0.3, std=1.7):
    from cofii2p_amd import autograd as ag

    g = torch.Generator(device=DEV).manual_seed(M + C + groups)
    x = torch.randn((M, C), device=DEV, generator=g) * std + mean
    ga = (1 + 0.2 * torch.randn((C,), device=DEV, generator=g)) if affine else None
    be = (0.3 * torch.randn((C,), device=DEV, generator=g)) if affine else None
    r = torch.randn((M, C), device=DEV, generator=g) if res else None
    dy = torch.randn((M, C), device=DEV, generator=g)
    fs = fx = None
    if fixed:
        rm, rv = torch.randn((C,), device=DEV, generator=g) * 0.2 + mean, (torch.rand((C,), device=DEV, generator=g) + 0.5) * std * std
        fs, fx = torch.stack([rm, torch.rsqrt(rv + 1e-5)], 1).contiguous(), (rm, rv)

    def run():
        ins = [t.clone().requires_grad_() if t is not None else None for t in (x, ga, be, r)]
        y = ag.group_norm_act(ins[0], ins[1], ins[2], groups, slope, ins[3], fixed_stats=fs)
        send(y, dy, strided)
        return (y.detach(), *[t.grad for t in ins if t is not None])

    out = same_twice(run)
    names = [n for n, t in zip(("x", "gamma", "beta", "res"), (x, ga, be, r)) if t is not None]
    yr, gr = _gn_reference(x, ga, be, r, groups, slope, fx, dy, torch.float64)
    return out, names, yr, [t for t in gr if t is not None], (x, ga, be, r, fx, dy)


GN_ROWS = [2, 5, 13, 16, 17, 29, 256, 257, 20100, 40000]
GN_CASES = (
    # rows: 13 / 16 / 17 / 29 sit around the four-rows-in-flight loop (m + 12 < r1), 256 | 257 around one | two row blocks, 20100 has an empty
    # last row block (156 x 129 > 20100), 40000 runs at the cap of 256 row blocks
    [(M, 64, 32, True, (0.1, 0.0, 1.0)[i % 3], i % 2 == 1, False, False) for i, M in enumerate(GN_ROWS)]
    + [(17, 64, 32, False, 0.1, False, False, False), (257, 64, 64, True, 0.0, True, True, False), (20100, 64, 32, False, 1.0, True, False, False),
       (29, 64, 64, True, 1.0, False, True, False), (257, 64, 32, True, 0.1, True, False, True)]
    # widths: C % 64 != 0 (the finalize kernel's group shuffles reach lanes with c >= C), one group, groups == C, 64 channels per group
    + [(300, 4, 1, True, 0.0, False, False, False), (300, 4, 4, False, 0.1, True, False, False), (300, 72, 18, True, 1.0, True, False, False),
       (300, 136, 136, True, 0.0, False, True, False), (300, 136, 136, False, 0.1, False, False, True), (300, 2048, 32, True, 0.1, False, False, False),
       (300, 72, 18, True, 0.1, False, False, True)]
)


@pytest.mark.parametrize("M,C,groups,affine,slope,res,fixed,strided", GN_CASES)
def test_group_norm_act_row_blocks_and_widths(M, C, groups, affine, slope, res, fixed, strided):
    out, names, yr, gr, _ = _gn_run(M, C, groups, affine, slope, res, fixed, strided)
    # measured on MI355X over all cases: forward <= 6.8e-8, gradients <= 1.9e-7
    print("group norm", (M, C, groups), "y %.2e" % rel_err(out[0], yr), " ".join("%s %.2e" % (n, rel_err(a, b)) for n, a, b in zip(names, out[1:], gr)))
    assert rel_err(out[0], yr) < 1e-5
    for n, a, b in zip(names, out[1:], gr):
        assert rel_err(a, b) < 2e-5, n


def test_group_norm_act_refuses_three_channels_per_group():
    from cofii2p_amd import _lib, autograd as ag

    x = torch.randn((300, 96), device=DEV, requires_grad=True)
    with pytest.raises(_lib.CofiError):
        ag.group_norm_act(x, None, None, 32, 0.1).backward(torch.ones((300, 96), device=DEV))


def test_group_norm_act_far_from_zero():
    """x ~ N(50, 0.5^2): the centred values lose 7 bits to the mean.  Plain fp32 torch autograd is itself about 2e-5 off float64 on dgamma
    here, so each quantity is allowed max(project tolerance, 4 x the error of fp32 torch on the same inputs) - that error is computed
    here, from torch alone.  Factor 4: two fp32 evaluations of one formula differ by about twice either's error, and the kernel's
    summation order is not torch's.  No activation (slope 1): with y known to 6e-6 only, an entry that close to zero takes the other
    branch of a LeakyReLU than the float64 reference's - a jump of the reference, not an error of the kernel (one such entry of 19200
    moved dbeta by 7e-3 when this case ran with slope 0.1)."""
    M, C, groups, slope = 300, 64, 32, 1.0
    out, names, yr, gr, (x, ga, be, r, fx, dy) = _gn_run(M, C, groups, True, slope, False, False, False, mean=50.0, std=0.5)
    y32, g32 = _gn_reference(x.cpu(), ga.cpu(), be.cpu(), None, groups, slope, None, dy.cpu(), torch.float32)
    e32 = [rel_err(y32, yr)] + [rel_err(a, b) for a, b in zip([t for t in g32 if t is not None], gr)]
    mine = [rel_err(out[0], yr)] + [rel_err(a, b) for a, b in zip(out[1:], gr)]
    # measured on MI355X: kernel y 5.5e-6, dx 1.7e-7, dgamma 2.2e-6, dbeta 1.4e-7; fp32 torch y 4.0e-6, dx 8.4e-7, dgamma 2.0e-5, dbeta 1.4e-7 -
    # the kernel (fp64 fold of the row-block partials) stays inside the plain tolerances
    print("group norm at N(50, 0.5^2): kernel", ["%.2e" % e for e in mine], "fp32 torch", ["%.2e" % e for e in e32])
    for n, tol, e, e0 in zip(["y"] + names, [1e-5, 2e-5, 2e-5, 2e-5], mine, e32):
        assert e < max(tol, 4.0 * e0), (n, e, e0)


# ------------------------------------------------------------------------------------------ 6. column sums, linear, column normalise
@pytest.mark.parametrize("C", [1, 64, 65, 130])
@pytest.mark.parametrize("M,view", [(1, False), (256, False), (257, False), (1000, False), (33000, False), (257, True), (33000, True)])
def test_col_sum_row_blocks(M, C, view):
    """every bias gradient: one row block (M <= 256), two, seven, and the cap of 256 (M > 32896) with 129 rows each"""
    from cofii2p_amd import autograd as ag

    g = torch.Generator(device=DEV).manual_seed(M + C)
    wide = torch.randn((M, C + 7), device=DEV, generator=g) + 0.5
    x = wide[:, 3:3 + C] if view else wide[:, 3:3 + C].contiguous()
    a, b = ag.col_sum(x), ag.col_sum(x)
    assert torch.equal(a, b)
    ref, mag = x.double().sum(0), x.double().abs().sum(0)
    assert rel_err(a, ref) < 1e-5
    assert float(((a.double() - ref).abs() / mag).max()) < 1e-5     # column by column, against what the column sums in magnitude


@pytest.mark.parametrize("M,K,N,strided", [(300, 64, 32, False), (33000, 8, 4, False), (300, 64, 32, True), (33000, 8, 4, True)])
def test_linear_bias_gradient_over_many_row_blocks(M, K, N, strided):
    from cofii2p_amd import autograd as ag

    g = torch.Generator(device=DEV).manual_seed(M)
    x, w = torch.randn((M, K), device=DEV, generator=g), torch.randn((N, K), device=DEV, generator=g) / math.sqrt(K)
    b, dy = torch.randn((N,), device=DEV, generator=g), torch.randn((M, N), device=DEV, generator=g) + 0.25

    def run():
        ins = [t.clone().requires_grad_() for t in (x, w, b)]
        y = ag.linear(*ins)
        send(y, dy, strided)
        return (y.detach(), *[t.grad for t in ins])

    out = same_twice(run)
    ref = [t.double().clone().requires_grad_() for t in (x, w, b)]
    yr = ref[0] @ ref[1].t() + ref[2]
    yr.backward(dy.double())
    assert rel_err(out[0], yr) < 1e-5
    for a, r, n in zip(out[1:], ref, ("x", "w", "bias")):
        assert rel_err(a, r.grad) < 1e-5, n


@pytest.mark.parametrize("C", [4, 65])
@pytest.mark.parametrize("L,strided", [(1, False), (257, False), (4100, False), (257, True), (4100, True)])
def test_normalize_cols_row_blocks(L, C, strided):
    """F.normalize(x, dim=0): one row (the exact gradient is zero), two row blocks, 32 row blocks with a short last one; C = 65: a second,
    one-column chunk.  Tolerances of test_normalize_cols_function."""
    from cofii2p_amd import autograd as ag

    g = torch.Generator(device=DEV).manual_seed(L + C)
    base = torch.randn((L, C + 8), device=DEV, generator=g)
    if L > 1:
        base[:, 4 + 2] = 0.0                                             # a dead column: clamped norm, y = 0, dx = dy / eps
    dy = torch.randn((L, C), device=DEV, generator=g)
    if L > 1:
        dy[:, 2] = 0.0

    def run():
        x = base.clone().requires_grad_()
        y = ag.normalize_cols(x[:, 4:4 + C])
        send(y, dy, strided)
        return y.detach(), x.grad[:, 4:4 + C].contiguous()

    y, dx = same_twice(run)
    xr = base.double().clone().requires_grad_()
    yr = F.normalize(xr[:, 4:4 + C], dim=0)
    yr.backward(dy.double())
    assert rel_err(y, yr) < 2e-6
    if L == 1:
        # y = sign(x): dx = dy / |x| - x (dy x) / |x|^3 = 0; judged against the size of the two terms that cancel
        assert bool((dx.abs() <= 5e-6 * (dy / base[:, 4:4 + C]).abs()).all())
    else:
        assert rel_err(dx, xr.grad[:, 4:4 + C]) < 5e-6
        assert float(y[:, 2].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------ 7. row normalise
@pytest.mark.parametrize("C", [100, 260])
@pytest.mark.parametrize("strided", [False, True])
def test_normalize_rows_tiny_and_clamped_rows(C, strided):
    """one row of norm ~1e-11 (just above eps = 1e-12: the full formula with 1 / n^3 ~ 1e33) and one of norm ~1e-13 (clamped: dx = dy / eps)
    with a NON-zero dy; their gradients are ~1e12 times the others', so they are judged one by one"""
    from cofii2p_amd import autograd as ag

    g = torch.Generator().manual_seed(C)
    M = 37
    base, dy = torch.randn((M, C), generator=g), torch.randn((M, C), generator=g)
    base[5] *= 1e-12
    base[9] *= 1e-14
    base[11] = 0.0

    def run():
        x = G(base.clone(), grad=True)
        y = ag.normalize_rows(x)
        send(y, G(dy), strided)
        return y.detach(), x.grad

    y, dx = same_twice(run)
    xr = base.double().clone().requires_grad_()
    yr = F.normalize(xr, dim=1)
    yr.backward(dy.double())
    assert float(base[5].double().norm()) > 1e-12 > float(base[9].double().norm()) > 0.0
    rest = [m for m in range(M) if m not in (5, 9, 11)]
    assert rel_err(y, yr) < 1e-6
    assert rel_err(dx.cpu()[rest], xr.grad[rest]) < 2e-6
    for m in (5, 9, 11):
        assert rel_err(y.cpu()[m], yr[m]) < 1e-6 or m == 11, m
        assert rel_err(dx.cpu()[m], xr.grad[m]) < 2e-6, (m, rel_err(dx.cpu()[m], xr.grad[m]))
    assert float(y[11].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------ 8. convolution operand
@pytest.mark.parametrize("H,W,Cin,Cout,ks,stride,pad", [(7, 9, 4, 8, 7, 2, 3), (5, 1, 4, 4, 3, 1, 1), (1, 6, 8, 4, 3, 1, 1), (6, 6, 4, 4, 3, 2, 0), (8, 8, 4, 4, 2, 2, 0)])
def test_conv_operand_geometries(H, W, Cin, Cout, ks, stride, pad):
    """a kernel as large as the map, one-pixel-wide and one-pixel-high maps, a stride that leaves the last row and column untouched, an even
    kernel: im2col / col2im alone against F.unfold, and the convolution built on them against F.conv2d"""
    from cofii2p_amd import autograd as ag

    g = torch.Generator(device=DEV).manual_seed(H * W + ks)
    x = torch.randn((1, Cin, H, W), device=DEV, generator=g)
    w = torch.randn((Cout, Cin, ks, ks), device=DEV, generator=g) / math.sqrt(Cin * ks * ks)
    Ho, Wo = (H + 2 * pad - ks) // stride + 1, (W + 2 * pad - ks) // stride + 1
    dcol = torch.randn((Ho * Wo, ks * ks * Cin), device=DEV, generator=g)
    dy = torch.randn((Ho * Wo, Cout), device=DEV, generator=g)
    rows = x.reshape(Cin, -1).t().contiguous()

    def run_operand():
        x1 = rows.clone().requires_grad_()
        col = ag.im2col(x1, H, W, ks, stride, pad)
        backward_through_cat(col, dcol)
        return col.detach(), x1.grad

    col, dx = same_twice(run_operand)
    x2 = x.double().clone().requires_grad_()
    unf = F.unfold(x2, ks, padding=pad, stride=stride)                                     # (1, Cin ks ks, Ho Wo), channel-major
    colr = unf.reshape(Cin, ks * ks, Ho * Wo).permute(2, 1, 0).reshape(Ho * Wo, ks * ks * Cin)   # column (dy ks + dx) Cin + c
    colr.backward(dcol.double())
    dxr = x2.grad[0].reshape(Cin, -1).t()
    assert torch.equal(col.double(), colr.detach())                                         # a copy
    assert rel_err(dx, dxr) < 1e-6                                                          # a gather of at most ks^2 terms
    untouched = (dxr.abs().sum(1) == 0)
    assert float(dx[untouched].abs().sum()) == 0.0
    if (H, ks, stride, pad) == (6, 3, 2, 0):
        assert int(untouched.sum()) == 11 and bool(untouched.reshape(H, W)[5].all()) and bool(untouched.reshape(H, W)[:, 5].all())

    def run_conv():
        x1, w1 = rows.clone().requires_grad_(), w.clone().requires_grad_()
        y, ho, wo = ag.conv2d(x1, H, W, w1, stride, pad)
        assert (ho, wo) == (Ho, Wo)
        y.backward(dy)
        return y.detach(), x1.grad, w1.grad

    y, dx, dw = same_twice(run_conv)
    x3, w3 = x.double().clone().requires_grad_(), w.double().clone().requires_grad_()
    yr = F.conv2d(x3, w3, None, stride, pad)
    yr.backward(dy.t().reshape(1, Cout, Ho, Wo).double())
    assert rel_err(y, yr[0].reshape(Cout, -1).t()) < 1e-5
    assert rel_err(dw, w3.grad) < 1e-5
    assert rel_err(dx, x3.grad[0].reshape(Cin, -1).t()) < 1e-5
    assert float(dx[untouched].abs().sum()) == 0.0


# ------------------------------------------------------------------------------------------ 9. up-sampling adjoint
def test_upsample2x_adjoint_grid_stride_loop():
    """72 x 240 x 512 channels: 2,211,840 work items of 4 channels, more than the 8192 x 256 threads of the capped grid - every thread takes a
    second element.  Reference: F.interpolate in float64 on the GPU."""
    from cofii2p_amd import autograd as ag

    h, w, C1, C2 = 72, 240, 512, 4
    assert h * w * C1 // 4 > 8192 * 256
    g = torch.Generator(device=DEV).manual_seed(9)
    low, skip = torch.randn((h * w, C1), device=DEV, generator=g), torch.randn((4 * h * w, C2), device=DEV, generator=g)
    dy = torch.randn((4 * h * w, C1 + C2), device=DEV, generator=g)

    def run():
        l, s_ = low.clone().requires_grad_(), skip.clone().requires_grad_()
        y = ag.upsample2x_cat(l, s_, h, w)
        y.backward(dy)
        return y.detach(), l.grad, s_.grad

    y, dl, ds = same_twice(run)
    lr = low.double().requires_grad_()
    up = F.interpolate(lr.t().reshape(1, C1, h, w), scale_factor=2, mode="bilinear", align_corners=False)
    upr = up.reshape(C1, 4 * h * w).t()
    upr.backward(dy[:, :C1].double())
    assert rel_err(y[:, :C1], upr) < 1e-6 and torch.equal(y[:, C1:], skip)
    assert rel_err(dl, lr.grad) < 1e-6
    rows = [0, w - 1, h * w // 2, 8192 * 256 * 4 // C1, h * w - w, h * w - 1]       # corners, and the first pixel of the second sweep
    assert_rows(dl[rows], lr.grad[rows], 1e-6, range(len(rows)))
    assert torch.equal(ds, dy[:, C1:])
