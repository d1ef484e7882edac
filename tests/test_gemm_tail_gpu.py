"""The tail of the MFMA-tile GEMM kernels (mfma32_tile_tail of csrc/gemm.hip and the copies three kernels keep of their own) - split-K
partial store, accumulators -> 64-row LDS slab -> row-wise epilogue, and the lean slab loop of the 256-row kernels - at the smallest
shapes at which it can go wrong, for each of the five kernel families, forced through the tuning hooks (include/cofi_hip_tune.h):

    f32       gemm_kernel                     tiles 128 x 128 (two 64-row halves), 64 x 128 and 64 x 64 (whole tile)
    x6_small  gemm_bf16x3_kernel<X6>          ... and 128 x 64
    planes    gemm_planes_kernel              all nine configurations (64 ... 256-row tiles, 256 / 512 threads)
    x6_big    gemm_x6_big_kernel              256 x 128, lean slab loop
    f16_big   gemm_f16_big_kernel             256 x 128 (fp32 W, eight waves) and 128 x 128 (pre-split W): lean slab loop with NS = 4 / 2

M = 65: slab 1 of the tile is partial and, in a 256-row tile, slabs 2 - 3 are dead (the barrier pairing of a dead slab, statistics on);
M = 257: a second tile with one live row; M = 333.  N = 132: the last column tile fails n0 + BN <= N and takes the generic slab loop while
its neighbour takes the lean one; N = 64 / 128: whole tiles.  K = 64 un-split, K = 256 split in two (partial store + splitk_epilogue_kernel).
Epilogue operands: EPILOGUES below.

Shapes a family refuses, and the nearest shape used instead:
  * the 256 x 128 kernels serve M >= 256 and N >= 128 (gemm_planner.h big_plan): M = 65 becomes 256 + 65 = 321 - the LAST tile has the
    65 rows, its slab 1 partial and its slabs 2 - 3 dead - and N = 64 is left out for them;
  * K splits come in chunks of 128 (split_k): K = 128 cannot be split in two, K = 256 is the smallest K that can.

Each case asserts
  (a) bit equality where the project states it for the pair: x6_big against the forced 128 x 128 register-staged plan at the same K split
      (output and statistics partials: test_big_tiles_bf16x6); planes against the register-staged kernel on the same pre-split operands
      (output bit for bit, statistics to rounding - the row-pass order of the fold depends on the workgroup shape:
      test_gemm_planes_gpu.py); the register-staged tiles among themselves (same products in the same K order: output bit for bit, statistics
      bit for bit at equal tile width, as test_tall_tiles_for_narrow_outputs_bf16x6 states for 128 x 64 against 64 x 64);
  (b) the error against a float64 evaluation of the same epilogue, in units of the magnitudes that enter an element,
      scale = |a| |w| / rowdiv + |bias| + |residual|  (= |a| |w| + |bias| without those operands): 2e-6 for the six-product and f16x3 kernels
      (test_big_tiles_bf16x6 / _f16x3), 3e-5 for the three-product planes kernel (test_gemm_bf16x3_split; the raw product also within 2e-5 of
      max |ref|, test_gemm_planes_gpu.py), rtol = atol = 2e-4 for fp32 (test_gemm).  LeakyReLU is 1-Lipschitz: a bound that holds before
      the activation holds behind it.  The tolerances are those tests'; the scale with the rowdiv and residual terms is this test's own
      form - no other test states it - and reduces to theirs, |a| |w| + |bias|, for the bias-only epilogue;
  (c) the statistics partials are the column sums of the stored values per 64-row slab (1e-3, as test_gemm_indexed_residual_gpu.py), and
      the sums of squares likewise within 1e-3 of the largest of them: that second, relative bound is this test's own (64 fp32 additions
      carry at most 63 * 2^-24 = 3.8e-6 of the sum).
The f16x3 family has no partner kernel that forms the same products, so the bit-exactness of ITS tail is not guarded by a committed test:
(b) and (c) catch a wrong slab, row, column or dead-slab mix-up, not a difference of the order of the rounding.
Needs a real MI355X:  python -m pytest tests -m gpu"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RES_ROWS = 50
# COFI_PLAN_* of include/cofi_hip_tune.h
PLAN_F32, PLAN_BF16X6, PLAN_PLANES, PLAN_BIG_X6, PLAN_BIG_F16, PLAN_BIG_F16_128 = 0, 2, 3, 4, 5, 7
NUM_PLANES_CFG = 9   # kPlanesCfg of csrc/gemm_planner.h

# (bias, rowdiv, LeakyReLU, statistics, residual: None | "plain" | "indexed")
EPILOGUES = [(True, False, False, False, None),
             (True, True, True, True, "plain"),
             (True, True, False, True, "indexed"),
             (False, False, True, False, "plain"),
             (False, False, True, True, None)]
KSPLITS = [(64, 1), (256, 2)]
SMALL_MN = [(M, N) for M in (65, 257, 333) for N in (64, 128, 132)]
BIG_MN = [(M, N) for M in (321, 257, 333) for N in (128, 132)]


@pytest.fixture(scope="module")
def env():
    from cofii2p_amd import _lib, ops

    assert torch.cuda.is_available()
    lib = _lib.load()
    for name, (restype, argtypes) in _lib.TUNE_SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    saved = ops.GEMM_MODE, ops.F16X3_BIG
    yield ops, lib
    _force(lib)
    ops.GEMM_MODE, ops.F16X3_BIG = saved


def _force(lib, plan=(0, 0, 0), planes=(-1, 0), big=(0, 0)):
    assert lib.cofi_tune_force_plan(*plan) == 0 and lib.cofi_tune_force_planes(*planes) == 0 and lib.cofi_tune_force_big(*big) == 0


def _planned(lib, M, N, K, flags):
    """what the planner - under the calling thread's overrides - gives this contraction: (family, bm, bn, ksplit)"""
    from cofii2p_amd._lib import PlanDesc

    d = PlanDesc()
    assert lib.cofi_tune_describe_gemm(M, N, K, flags, 0, 0, 1, 1 << 30, ctypes.byref(d)) == 0
    return d.family, d.bm, d.bn, d.ksplit


_CASES = {}


def _case(M, N, K):
    """operands of one shape and the float64 results of every epilogue: computed once, shared by the families, never written to"""
    if (M, N, K) in _CASES:
        return _CASES[(M, N, K)]
    g = torch.Generator().manual_seed(1000 * M + 10 * N + K)
    a = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) / K ** 0.5
    bias = torch.randn(N, generator=g)
    rowdiv = torch.randint(1, 9, (M,), generator=g).float()
    rowdiv[M - 1] = 7.0   # the last row's divisor is the one a clamped load past M reads
    res = torch.randn(M, N, generator=g)
    src = torch.randn(RES_ROWS, N, generator=g)
    idx = torch.randint(0, RES_ROWS, (M,), generator=g, dtype=torch.int32)
    idx[::17] = RES_ROWS   # shadow entries: zero residual
    idx[M - 1] = -1
    ok = (idx >= 0) & (idx < RES_ROWS)
    gathered = torch.where(ok[:, None], src[idx.clamp(0, RES_ROWS - 1).long()], torch.zeros(M, N))
    prod = a.double() @ w.double().t()
    mag = a.double().abs() @ w.double().abs().t()
    refs = []
    for has_bias, has_rd, leaky, _, rkind in EPILOGUES:
        r = {None: None, "plain": res, "indexed": gathered}[rkind]
        x, s = prod, mag
        if has_rd:
            x, s = x / rowdiv[:, None].double(), s / rowdiv[:, None].double()
        if has_bias:
            x, s = x + bias.double(), s + bias.double().abs()
        if r is not None:
            x, s = x + r.double(), s + r.double().abs()
        if leaky:
            x = torch.where(x >= 0, x, x * 0.1)
        refs.append((x, s))
    c = dict(a=a.to(DEV), w=w.to(DEV), bias=bias.to(DEV), rowdiv=rowdiv.to(DEV), res=res.to(DEV), src=src.to(DEV), idx=idx.to(DEV),
             prod=prod, refs=refs)
    _CASES[(M, N, K)] = c
    return c


def _run(ops, c, a, w, e):
    """the launch of epilogue e -> (output, statistics partials or None)"""
    has_bias, has_rd, leaky, stats, rkind = EPILOGUES[e]
    kw = dict(bias=c["bias"] if has_bias else None, rowdiv=c["rowdiv"] if has_rd else None, act=ops.ACT_LEAKY01 if leaky else ops.ACT_NONE)
    if rkind == "plain":
        kw.update(res=c["res"])
    elif rkind == "indexed":
        kw.update(res=c["src"], res_idx=c["idx"])
    if stats:
        y, part = ops.gemm_colstats(a, w, **kw)
        return y.clone(), part.clone()
    return ops.gemm(a, w, **kw).clone(), None


def _check_against_fp64(c, e, y, part, tol, what):
    ref, scale = c["refs"][e]
    yc = y.double().cpu()
    if tol == "f32":   # test_gemm's bound
        err = float(((yc - ref).abs() - 2e-4 * ref.abs()).max())
        print(what, "fp32 |y - ref| - rtol |ref| =", err)
        assert err <= 2e-4, (what, err)
    else:
        err = float(((yc - ref).abs() / scale).max())
        print(what, "scaled error", err)
        assert err < tol, (what, err)
    if part is not None:
        M = yc.shape[0]
        assert part.shape[0] == (M + 63) // 64, what
        sums = torch.stack([yc[s:s + 64].sum(0) for s in range(0, M, 64)])
        sqs = torch.stack([yc[s:s + 64].pow(2).sum(0) for s in range(0, M, 64)])
        es, eq = float((part[:, :, 0].double().cpu() - sums).abs().max()), float((part[:, :, 1].double().cpu() - sqs).abs().max())
        print(what, "statistics: sum", es, "sum of squares", eq)
        assert es < 1e-3 and eq < 1e-3 * max(1.0, float(sqs.abs().max())), (what, es, eq)


def _register_staged(env, mode, family, flags, tiles, tol):
    ops, lib = env
    ops.GEMM_MODE, ops.F16X3_BIG = mode, False
    try:
        for M, N in SMALL_MN:
            for K, ks in KSPLITS:
                c = _case(M, N, K)
                for e in range(len(EPILOGUES)):
                    got = {}
                    for bm, bn in tiles:
                        _force(lib, plan=(bm, bn, ks), big=(-1, 0))
                        assert _planned(lib, M, N, K, flags) == (family, bm, bn, ks)
                        got[(bm, bn)] = _run(ops, c, c["a"], c["w"], e)
                        _check_against_fp64(c, e, *got[(bm, bn)], tol, (mode, bm, bn, M, N, K, ks, e))
                    for (bm, bn), (y, part) in got.items():
                        assert torch.equal(y, got[(128, 128)][0]), (mode, bm, bn, M, N, K, ks, e)
                        if part is not None and (128, bn) in got:   # equal tile width: the same fold order
                            assert torch.equal(part, got[(128, bn)][1]), (mode, bm, bn, M, N, K, ks, e)
    finally:
        _force(lib)


def test_tail_f32(env):
    """gemm_kernel: 128 x 128 (two halves), 64 x 128 and 64 x 64 (whole tile)"""
    _register_staged(env, "f32", PLAN_F32, 0, [(128, 128), (64, 128), (64, 64)], "f32")


def test_tail_x6_small(env):
    """gemm_bf16x3_kernel, six products: every tile it is built for.  The 128 x 128 plan is the reference of test_tail_x6_big."""
    from cofii2p_amd import ops

    _register_staged(env, "bf16x6", PLAN_BF16X6, ops.GEMM_BF16X6, [(128, 128), (64, 128), (128, 64), (64, 64)], 2e-6)


def test_tail_planes(env):
    """gemm_planes_kernel, every configuration, against the register-staged kernel on the same planes at the same K split"""
    ops, lib = env
    ops.GEMM_MODE, ops.F16X3_BIG = "bf16x3", False
    flags = ops.GEMM_BF16X3 | ops.GEMM_W_SPLIT | ops.GEMM_A_SPLIT
    try:
        for M, N in SMALL_MN:
            for K, ks in KSPLITS:
                c = _case(M, N, K)
                sw = ops.SplitW(c["w"])
                sa = ops.SplitA(ops.SplitW(c["a"]).planes, K)   # the library's own split (cofi_split_bf16_planes)
                for e in range(len(EPILOGUES)):
                    _force(lib, plan=(64, 64, ks), planes=(-2, 0))
                    y0, part0 = _run(ops, c, sa, sw, e)
                    raw0 = ops.gemm(sa, sw).clone()
                    if e == 0:
                        err = float((raw0.double().cpu() - c["prod"]).abs().max() / c["prod"].abs().max())
                        assert err < 2e-5, (M, N, K, ks, err)
                    for cfg in range(NUM_PLANES_CFG):
                        _force(lib, planes=(cfg, ks))
                        fam, _, _, got_ks = _planned(lib, M, N, K, flags)
                        assert (fam, got_ks) == (PLAN_PLANES, ks)
                        what = ("planes", cfg, M, N, K, ks, e)
                        y, part = _run(ops, c, sa, sw, e)
                        assert torch.equal(y, y0), what
                        if part is not None:
                            assert torch.allclose(part, part0, rtol=2e-5, atol=1e-3), what
                        if e == 0:
                            assert torch.equal(ops.gemm(sa, sw), raw0), what
                        _check_against_fp64(c, e, y, part, 3e-5, what)
    finally:
        _force(lib)


def test_tail_x6_big(env):
    """gemm_x6_big_kernel against the forced 128 x 128 register-staged plan at the same K split: output and statistics bit for bit"""
    ops, lib = env
    ops.GEMM_MODE, ops.F16X3_BIG = "bf16x6", False
    try:
        for M, N in BIG_MN:
            for K, ks in KSPLITS:
                c = _case(M, N, K)
                for e in range(len(EPILOGUES)):
                    what = ("x6_big", M, N, K, ks, e)
                    _force(lib, big=(1, ks))
                    assert _planned(lib, M, N, K, ops.GEMM_BF16X6) == (PLAN_BIG_X6, 256, 128, ks)
                    y, part = _run(ops, c, c["a"], c["w"], e)
                    _force(lib, plan=(128, 128, ks), big=(-1, 0))
                    y0, part0 = _run(ops, c, c["a"], c["w"], e)
                    assert torch.equal(y, y0), what
                    if part is not None:
                        assert torch.equal(part, part0), what
                    _check_against_fp64(c, e, y, part, 2e-6, what)
    finally:
        _force(lib)


@pytest.mark.parametrize("presplit", [False, True])
def test_tail_f16_big(env, presplit):
    """gemm_f16_big_kernel: fp32 W (256 x 128, eight waves) and pre-split W (128 x 128, four waves, two workgroups per CU).  No other kernel
    forms the same products, so nothing here compares bits with another kernel (module docstring): (b), (c), the launch really ran on this
    kernel, nothing went to the repair launch, two runs give equal bits."""
    ops, lib = env
    ops.GEMM_MODE, ops.F16X3_BIG = "bf16x6", True
    flags = ops.GEMM_BF16X6 | ops.GEMM_F16X3 | (ops.GEMM_W_F16PRE if presplit else 0)
    try:
        for M, N in BIG_MN:
            for K, ks in KSPLITS:
                c = _case(M, N, K)
                w = ops.presplit(c["w"]) if presplit else c["w"]
                for e in range(len(EPILOGUES)):
                    what = ("f16_big", presplit, M, N, K, ks, e)
                    _force(lib, big=(1, ks))
                    assert _planned(lib, M, N, K, flags) == ((PLAN_BIG_F16_128, 128, 128, ks) if presplit else (PLAN_BIG_F16, 256, 128, ks))
                    lib.cofi_tune_f16x3_launch_flops(1, None)
                    lib.cofi_tune_f16x3_resplit_events(1)
                    y, part = _run(ops, c, c["a"], w, e)
                    assert lib.cofi_tune_f16x3_launch_flops(1, None) == 1 and lib.cofi_tune_f16x3_resplit_events(1) == 0, what
                    if presplit:
                        assert w._f16pre is not None, "the launch did not take the pre-split weight"
                    y2, part2 = _run(ops, c, c["a"], w, e)
                    assert torch.equal(y, y2) and (part is None or torch.equal(part, part2)), what
                    _check_against_fp64(c, e, y, part, 2e-6, what)
    finally:
        _force(lib)
