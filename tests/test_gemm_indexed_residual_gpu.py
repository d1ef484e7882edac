"""The indexed residual of the GEMM epilogues (cofi_gemm_f32_fused_res, include/cofi_hip.h): output row m of frame f adds row
f * res_rows + res_idx[m] of a projected coarse level - zero for a shadow index - before activation, statistics and L2 normalisation.
Every kernel family that has an epilogue of its own is forced in turn; the results are compared BIT for bit with the same launch
given the materialised gather as a dense residual, and with the plain launch plus the gathered rows added by torch.
Needs a real MI355X:  python -m pytest tests -m gpu"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FRAMES, ROWS, RES_ROWS = 2, 256 + 40, 150   # two frames of 296 rows: ragged 64 / 128 / 256-row tiles, and tiles that straddle the frames
M = FRAMES * ROWS


@pytest.fixture(scope="module")
def ops():
    from cofii2p_amd import ops as _ops

    assert torch.cuda.is_available()
    saved = _ops.GEMM_MODE, _ops.F16X3_BIG
    yield _ops
    _ops.GEMM_MODE, _ops.F16X3_BIG = saved


def _hooks(ops):
    lib = ops._lib.load()
    fp, fb = lib.cofi_tune_force_plan, lib.cofi_tune_force_big
    fp.argtypes, fp.restype = [ctypes.c_int] * 3, ctypes.c_int
    fb.argtypes, fb.restype = [ctypes.c_int] * 2, ctypes.c_int
    return fp, fb


def _f16_launches(ops):
    fn = ops._lib.load().cofi_tune_f16x3_launch_flops
    fn.argtypes, fn.restype = [ctypes.c_int, ctypes.POINTER(ctypes.c_double)], ctypes.c_long
    return fn(1, None)


def _f16_events(ops):
    fn = ops._lib.load().cofi_tune_f16x3_resplit_events
    fn.argtypes, fn.restype = [ctypes.c_int], ctypes.c_long
    return fn(1)


def _index_table(g):
    """(M, 4) int32, column 0 in use (stride 4): frame-local rows of the projected level, 5 % shadow entries (== RES_ROWS, two of them
    negative).  Both frames draw from the whole range, so a launch that forgot the frame offset reads other rows for frame 1.  The unused
    columns hold values that are out of range for any reading."""
    idx = torch.randint(0, RES_ROWS, (M,), generator=g, dtype=torch.int32)
    shadow = torch.randperm(M, generator=g)[: M * 5 // 100]
    idx[shadow] = RES_ROWS
    idx[shadow[:2]] = -1
    tab = torch.full((M, 4), 1 << 20, dtype=torch.int32)
    tab[:, 0] = idx
    return tab


def _gathered(P, tab):
    """P[idx] by torch: frame-local indices, zero rows for shadow indices"""
    idx = tab[:, 0].long()
    ok = (idx >= 0) & (idx < RES_ROWS)
    frame = torch.arange(M) // ROWS
    rows = P[(frame * RES_ROWS + idx.clamp(0, RES_ROWS - 1))]
    return torch.where(ok[:, None], rows, torch.zeros_like(rows))


# family -> (arithmetic, f16x3 kernel, static W, force_plan, force_big, N, K, conv: a 1 x 1 convolution reaches the same kernel and plan)
FAMILIES = {
    "small_64x64": ("bf16x6", False, False, (64, 64, 1), (-1, 0), 64, 64, True),
    "small_128x128": ("bf16x6", False, False, (128, 128, 1), (-1, 0), 256, 256, True),
    "small_128x64": ("bf16x6", False, False, (128, 64, 1), (-1, 0), 64, 256, True),
    "small_128x128_f32": ("f32", False, False, (128, 128, 1), (-1, 0), 128, 64, True),
    "x6_big": ("bf16x6", False, False, (0, 0, 0), (1, 1), 256, 256, False),
    "f16_big_presplit_w": ("bf16x6", True, True, (0, 0, 0), (1, 1), 256, 256, False),
    "f16_big_f32_w": ("bf16x6", True, False, (0, 0, 0), (1, 1), 128, 64, False),
    "splitk_small": ("bf16x6", False, False, (64, 64, 2), (-1, 0), 128, 2048, True),
    "splitk_x6_big": ("bf16x6", False, False, (0, 0, 0), (1, 2), 256, 2048, False),
    "splitk_f16_big": ("bf16x6", True, False, (0, 0, 0), (1, 2), 256, 2048, False),
}


@pytest.mark.parametrize("family", list(FAMILIES))
def test_indexed_residual_equals_dense_residual(ops, family):
    """(1) no activation, no statistics: the output is the plain launch's output plus P[idx] added by torch in fp32.
    (2) LeakyReLU + column statistics: output and statistics partials equal, bit for bit, the dense-residual launch at the same plan
        given the gather materialised by cofi_gather_rows - through cofi_conv2d_nhwc_fused as a 1 x 1 convolution where that entry
        reaches the kernel (the small tiles and their split-K fold), and for the 256 x 128 kernels, which a 1 x 1 convolution never
        takes, through the same entry with res_idx == NULL (the dense residual load these kernels have had since the image branch).
    (3) the f16x3 families really ran on that kernel."""
    mode, f16, static_w, plan, big, N, K, conv = FAMILIES[family]
    ops.GEMM_MODE, ops.F16X3_BIG = mode, f16
    fp, fb = _hooks(ops)
    g = torch.Generator().manual_seed(sum(map(ord, family)))
    a = torch.randn(M, K, generator=g).to(DEV)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(DEV)
    bias = torch.randn(N, generator=g).to(DEV)
    P_cpu = torch.randn(FRAMES * RES_ROWS, N, generator=g)
    tab_cpu = _index_table(g)
    P, tab = P_cpu.to(DEV), tab_cpu.to(DEV)
    wd = ops.presplit(w) if static_w else w
    try:
        assert fp(*plan) == 0 and fb(*big) == 0
        dense = ops.gather_rows(P, tab, frames=FRAMES)
        assert torch.equal(dense.cpu(), _gathered(P_cpu, tab_cpu))
        _f16_launches(ops)
        plain = ops.gemm(a, wd, bias=bias, frames=FRAMES)
        got = ops.gemm(a, wd, bias=bias, frames=FRAMES, res=P, res_idx=tab)
        assert torch.equal(got, plain + dense), family
        # a 1-D table (stride 1) reads the same rows
        assert torch.equal(got, ops.gemm(a, wd, bias=bias, frames=FRAMES, res=P, res_idx=tab[:, 0].contiguous(), res_rows=RES_ROWS))
        y, part = ops.gemm_colstats(a, wd, bias=bias, act=ops.ACT_LEAKY01, frames=FRAMES, res=P, res_idx=tab)
        n_f16 = _f16_launches(ops)
        if conv:
            y_ref, part_ref, _, _ = ops.conv2d_nhwc(a, M, 1, wd, 1, stride=1, pad=0, bias=bias, res=dense, act=ops.ACT_LEAKY01, colstats=True)
        else:
            y_ref, part_ref = ops.gemm_colstats(a, wd, bias=bias, act=ops.ACT_LEAKY01, frames=FRAMES, res=dense)
        assert torch.equal(y, y_ref) and torch.equal(part, part_ref), family
        assert n_f16 == (4 if f16 else 0), (family, n_f16)
        if static_w:
            assert wd._f16pre is not None, "the launch did not take the pre-split weight"
    finally:
        fp(0, 0, 0)
        fb(0, 0)
    # the statistics are those of the stored values, residual included
    yc = y.double().cpu()
    sums = torch.stack([yc[s:s + 64].sum(0) for s in range(0, M, 64)])
    assert part.shape[0] == sums.shape[0]
    assert float((part[:, :, 0].double().cpu() - sums).abs().max()) < 1e-3
    # and the sum is right against fp64
    ref = a.double().cpu() @ w.double().cpu().t() + bias.double().cpu() + _gathered(P_cpu, tab_cpu).double()
    assert float((got.double().cpu() - ref).abs().max()) < (2e-5 if mode == "bf16x6" else 1e-4) * max(1.0, K / 256)


def test_indexed_residual_in_f16x3_repair_tiles(ops):
    """Tiles that leave the fp16 window of their panel's scale are computed again by the ROBUST instantiation of gemm_f16_big_kernel: its
    epilogue adds the indexed residual as well.  A's late K-tiles carry entries 1e4 x larger than anything the first tile saw
    (test_f16x3_range_tracking's recipe)."""
    ops.GEMM_MODE, ops.F16X3_BIG = "bf16x6", True
    fp, fb = _hooks(ops)
    g = torch.Generator().manual_seed(5)
    N, K = 256, 1024
    a = torch.randn(M, K, generator=g)
    a[100, 20 * 32 + 5] = 3e4     # frame 0, row panel 0
    a[ROWS + 200, 25 * 32:] *= 1e4   # frame 1, last (ragged) row panel
    a = a.to(DEV)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(DEV)
    bias = torch.randn(N, generator=g).to(DEV)
    P = torch.randn(FRAMES * RES_ROWS, N, generator=g).to(DEV)
    tab = _index_table(g).to(DEV)
    try:
        assert fb(1, 1) == 0
        dense = ops.gather_rows(P, tab, frames=FRAMES)
        plain = ops.gemm(a, w, bias=bias, frames=FRAMES)
        _f16_events(ops)
        got = ops.gemm(a, w, bias=bias, frames=FRAMES, res=P, res_idx=tab)
        assert _f16_events(ops) > 0
        y, part = ops.gemm_colstats(a, w, bias=bias, act=ops.ACT_LEAKY01, frames=FRAMES, res=P, res_idx=tab)
        assert _f16_events(ops) > 0
        y_ref, part_ref = ops.gemm_colstats(a, w, bias=bias, act=ops.ACT_LEAKY01, frames=FRAMES, res=dense)
    finally:
        fb(0, 0)
    assert torch.equal(got, plain + dense)
    assert torch.equal(y, y_ref) and torch.equal(part, part_ref)


@pytest.mark.parametrize("mode,K", [("bf16x6", 256), ("bf16x3", 64), ("f32", 64)])
def test_indexed_residual_l2norm(ops, mode, K):
    """decoder2's form: N = 64 with the L2-normalising epilogue (the generic row-wise path) - unit rows, equal to
    F.normalize(plain + P[idx]) to 1e-6"""
    ops.GEMM_MODE, ops.F16X3_BIG = mode, True
    g = torch.Generator().manual_seed(K)
    N = 64
    a = torch.randn(M, K, generator=g).to(DEV)
    w = ops.presplit((torch.randn(N, K, generator=g) / K ** 0.5).to(DEV))
    bias = torch.randn(N, generator=g).to(DEV)
    P = torch.randn(FRAMES * RES_ROWS, N, generator=g).to(DEV)
    tab = _index_table(g).to(DEV)
    plain = ops.gemm(a, w, bias=bias, frames=FRAMES)
    got = ops.gemm(a, w, bias=bias, frames=FRAMES, l2norm=True, res=P, res_idx=tab)
    want = torch.nn.functional.normalize(plain + ops.gather_rows(P, tab, frames=FRAMES), dim=1)
    assert float((got.norm(dim=1) - 1).abs().max()) < 1e-6
    assert float((got - want).abs().max()) < 1e-6


def test_indexed_residual_argument_errors(ops):
    from cofii2p_amd.ops import _p, _stream

    lib = ops._lib.load()
    N, K = 64, 64
    a = torch.randn(M, K, device=DEV)
    w = torch.randn(N, K, device=DEV)
    out = torch.empty(M, N, device=DEV)
    P = torch.randn(FRAMES * RES_ROWS, N, device=DEV)
    idx = torch.zeros(M, dtype=torch.int32, device=DEV)

    def call(res=P, ldr=N, res_idx=idx, stride=1, res_rows=RES_ROWS, frames=FRAMES):
        return lib.cofi_gemm_f32_fused_res(_p(a), K, None, _p(w), K, _p(out), N, M, N, K, None, None, 0, None, 1, None, 0, frames,
                                           _p(res), ldr, _p(res_idx), stride, res_rows, _stream())

    EINVAL = -1
    assert call() == 0
    assert call(res=None) == EINVAL            # an index table without a residual
    assert call(ldr=N - 4) == EINVAL           # residual rows shorter than the output's
    assert call(res_idx=None, ldr=N - 4) == EINVAL
    assert call(res_rows=0) == EINVAL and call(res_rows=-3) == EINVAL
    assert call(frames=3) == EINVAL            # M % frames != 0
    assert call(stride=0) == EINVAL
    torch.cuda.synchronize()
    with pytest.raises(ops._lib.CofiError):
        ops.gemm(a, w, res_idx=idx)
