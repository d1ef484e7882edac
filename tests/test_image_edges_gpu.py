"""The implicit-GEMM convolution (csrc/gemm.hip conv_entry and the kernel families behind it) and the NHWC glue kernels (csrc/image.hip)
at the geometries where the row decode, the tap decode, the padding mask and the tile tails can go wrong, against the float64 references
of tests/image_refs.py - in every arithmetic ("f32", "bf16x3", "bf16x6"), with plain and pre-split weights, stacked frames, strided
operands, forced tile plans and split-K, the direct 3 x 3 kernel at its smallest maps and the pending-normalisation loader.

Error measure of the convolutions: max |out - ref| / abs_scale, abs_scale = the convolution of |x| with |w| (image_refs.abs_scale).
Bounds (none of them comes from a kernel under test):
  bf16x3       < 3e-5, the bound of test_gemm_bf16x3_split
  f32, bf16x6  < max(4 x the error of torch's own float32 CPU convolution of the same case against the float64 reference, 1e-6): two fp32
               evaluations in different summation orders differ by about twice either's error
Measured on an MI355X, largest error over the cases of this module, each with plain and pre-split weights:
  f32 5.1e-7 and bf16x6 7.5e-7 (5 x 1 map, bias + residual + ReLU: bound 2.0e-6, torch's float32 5.1e-7 - the rounding of the sum with a
  bias and a residual of size 1, measured against the much smaller sum of |products| of a 12-term contraction), bf16x3 8.5e-6 (the
  one-pixel map); no case above 0.37 of its bound.
  Pending normalisation: 1.7e-5 (bf16x3) and 6.1e-7 (bf16x6) absolute against the 3e-4 bound.

What runs what:
  nine edge geometries x four epilogue forms x arithmetic x weight form            test_conv_edge_geometries
  x / out= as column slices of wider buffers                                       test_conv_strided_input_and_output
  column statistics at frames = 1                                                  test_conv_column_statistics
  forced 64x64, 64x128, 128x128, 128x64 tiles and split-K                          test_conv_forced_plans
  the direct 3 x 3 kernel (2- and 4-row tiles, off, default) at 4 x 64 and 8 x 64   test_conv_direct_kernel_smallest_maps
  pending InstanceNorm + ReLU: fused loader and the materialising fallback         test_conv_pending_norm
  refusals before any launch                                                       test_conv_refusals
  max-pool, up-sampling + concatenation, the stem's im2col: edge maps, frames      test_maxpool_*, test_upsample_*, test_im2col_stem_*
  their grid-stride loops (more than 8192 x 256 work items)                        test_*_grid_stride_loop
  the wrappers' operand checks                                                     test_glue_wrappers_refuse_*
Needs a real MI355X:  python -m pytest tests/test_image_edges_gpu.py -m gpu"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import image_refs as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENT = 7.0
MODES = ["f32", "bf16x3", "bf16x6"]
X3_BOUND = 3e-5            # test_gemm_bf16x3_split; largest measured here 8.5e-6
F32_FLOOR, F32_FACTOR = 1e-6, 4.0      # f32 / bf16x6: max(4 x torch's float32 error, 1e-6); largest measured 5.1e-7 / 7.5e-7, torch's 5.1e-7
WORST = {}                 # arithmetic (and "torch f32") -> largest error seen, printed by every test


@pytest.fixture(scope="module")
def ops():
    from cofii2p_amd import ops as _ops

    assert torch.cuda.is_available()
    return _ops


@pytest.fixture(scope="module")
def CofiError():
    from cofii2p_amd._lib import CofiError as E

    return E


@pytest.fixture(scope="module")
def hooks(ops):
    lib = ops._lib.load()
    plan, direct = lib.cofi_tune_force_plan, lib.cofi_tune_force_conv_direct      # tuning hooks: state of the calling thread
    plan.argtypes, plan.restype = [ctypes.c_int] * 3, ctypes.c_int
    direct.argtypes, direct.restype = [ctypes.c_int], ctypes.c_int
    return plan, direct


def G(t):
    return t.to(DEV)


def gid(geom):
    return "x".join(str(v) for v in geom)


def wide_of(t, off=4, pad=8, fill=SENT):
    """(column block at `off` of a wider device buffer that holds t, the buffer); the buffer's width is a multiple of 4"""
    M, C = t.shape
    Wd = (off + C + pad + 3) // 4 * 4
    wide = torch.full((M, Wd), fill, device=DEV)
    wide[:, off:off + C] = t.to(DEV)
    return wide[:, off:off + C], wide


def close(got, ref, tol, what=""):
    np.testing.assert_allclose(got.detach().double().cpu().numpy(), ref.detach().double().cpu().numpy(), rtol=tol, atol=tol, err_msg=str(what))


def scaled_err(out, ref, scale):
    return float(((out.detach().double().cpu() - ref).abs() / scale).max())


def note(key, err):
    WORST[key] = max(WORST.get(key, 0.0), err)


def report():
    print("largest so far:", "  ".join("%s %.3g" % kv for kv in sorted(WORST.items())))


# ====================================================================================================================== convolution
FORMS = ["bare", "bias", "bias+res+relu", "act_col0"]
_cases = {}


def conv_case(geom):
    """inputs, float64 references per form, the error scale and torch's float32 error per form - computed once per geometry"""
    if geom in _cases:
        return _cases[geom]
    H, W, Cin, Cout, ks, stride, pad, frames = geom
    x, w, bias, res = R.conv_case(geom)
    c0 = Cout // 2
    ref = {
        "bare": R.conv2d_nhwc_ref(x, H, W, w, ks, stride, pad, frames=frames),
        "bias": R.conv2d_nhwc_ref(x, H, W, w, ks, stride, pad, bias, frames=frames),
        "bias+res+relu": R.conv2d_nhwc_ref(x, H, W, w, ks, stride, pad, bias, res, R.ACT_RELU, frames=frames),
        "act_col0": R.conv2d_nhwc_ref(x, H, W, w, ks, stride, pad, bias, None, R.ACT_RELU, c0, frames),
    }
    scale = R.abs_scale(x, H, W, w, ks, stride, pad, frames)
    # torch's own float32 convolution on the CPU, each form evaluated in float32 throughout
    t32 = R.to_rows(F.conv2d(R.to_nchw(x, H, W, frames), R.weight_oihw(w, ks), None, stride, pad))
    tb = t32 + bias
    f32 = {"bare": t32, "bias": tb, "bias+res+relu": torch.relu(tb + res), "act_col0": torch.cat([tb[:, :c0], torch.relu(tb[:, c0:])], 1)}
    base = {k: scaled_err(f32[k], ref[k], scale) for k in FORMS}
    for k in FORMS:
        note("torch f32", base[k])
    _cases[geom] = dict(x=x, w=w, bias=bias, res=res, ref=ref, scale=scale, base=base, dev=dict(x=G(x), w=G(w), bias=G(bias), res=wide_of(res)[0]))
    return _cases[geom]


def bound(mode, base):
    return X3_BOUND if mode == "bf16x3" else max(F32_FACTOR * base, F32_FLOOR)


def run_form(ops, geom, c, form, w, x=None, out=None, colstats=False):
    H, W, Cin, Cout, ks, stride, pad, frames = geom
    d = c["dev"]
    kw = dict(frames=frames, out=out, colstats=colstats)
    if form != "bare":
        kw["bias"] = d["bias"]
    if form == "bias+res+relu":
        kw.update(res=d["res"], act=ops.ACT_RELU)          # the residual is a column slice of a wider buffer
    if form == "act_col0":
        kw.update(act=ops.ACT_RELU, act_col0=Cout // 2)
    r = ops.conv2d_nhwc(d["x"] if x is None else x, H, W, w, ks, stride, pad, **kw)
    assert (r[-2], r[-1]) == (R.out_size(H, ks, stride, pad), R.out_size(W, ks, stride, pad))
    return r


def check_conv(ops, geom, c, form, mode, what, **kw):
    """plain and pre-split weights in one arithmetic: both inside the bound; bf16x3 / bf16x6: bit-equal to each other (as
    test_gemm_bf16x3_split / test_gemm_bf16x6_is_fp32_grade assert for the dense GEMM)"""
    d = c["dev"]
    with ops.arithmetic(mode):
        plain = run_form(ops, geom, c, form, d["w"], **kw)[0].clone()
        split = run_form(ops, geom, c, form, ops.presplit(d["w"]), **kw)[0].clone()
    b = bound(mode, c["base"][form])
    errs = [scaled_err(o, c["ref"][form], c["scale"]) for o in (plain, split)]
    print("conv %s %s %s %s: plain %.3g pre-split %.3g | bound %.3g (torch f32 %.3g)" % (gid(geom), form, mode, what, errs[0], errs[1], b, c["base"][form]))
    note(mode, max(errs))
    assert bool(torch.isfinite(plain).all()) and bool(torch.isfinite(split).all()), (geom, form, mode, what)
    assert errs[0] < b, (geom, form, mode, what, "plain weights", errs[0], b)
    assert errs[1] < b, (geom, form, mode, what, "pre-split weights", errs[1], b)
    if mode != "f32":
        assert torch.equal(plain, split), (geom, form, mode, what, "pre-split weights give other bits")
    return plain


@pytest.mark.parametrize("geom", R.CONV_GEOMS, ids=gid)
def test_conv_edge_geometries(ops, geom):
    c = conv_case(geom)
    for form in FORMS:
        for mode in MODES:
            check_conv(ops, geom, c, form, mode, "default plan")
    report()


@pytest.mark.parametrize("geom", [R.ROW6, R.CIN68], ids=gid)
def test_conv_strided_input_and_output(ops, geom):
    """x as the column block at offset 4 of a wider buffer; out= the column block at offset 4 of a zero-filled wider buffer, whose other
    columns must still be exactly zero"""
    H, W, Cin, Cout, ks, stride, pad, frames = geom
    c = conv_case(geom)
    xs, _ = wide_of(c["x"], off=4)
    M = c["ref"]["bare"].shape[0]
    for form in FORMS:
        for mode in MODES:
            dense = check_conv(ops, geom, c, form, mode, "dense")
            got = check_conv(ops, geom, c, form, mode, "x view", x=xs)
            assert torch.equal(got, dense), (geom, form, mode, "a strided x gives other bits")
            buf = torch.zeros((M, Cout + 12), device=DEV)
            got = check_conv(ops, geom, c, form, mode, "out view", out=buf[:, 4:4 + Cout])
            assert torch.equal(got, dense), (geom, form, mode, "a strided out gives other bits")
            assert float(buf[:, :4].abs().max()) == 0.0 and float(buf[:, 4 + Cout:].abs().max()) == 0.0, "the kernel wrote outside its column block"
    report()


@pytest.mark.parametrize("geom", [g for g in R.CONV_GEOMS if g[-1] == 1], ids=gid)
def test_conv_column_statistics(ops, geom):
    """colstats=True: the partials folded by group_stats_from_colpart (one group per column) against mean and rstd of the reference output,
    at the 1e-4 of test_gemm_fused_column_statistics; the output is the one the plain call gives"""
    H, W, Cin, Cout, ks, stride, pad, frames = geom
    c = conv_case(geom)
    for form in ("bias", "bias+res+relu"):
        ref = c["ref"][form]
        M = ref.shape[0]
        mean, rstd = ref.mean(0), 1.0 / torch.sqrt(ref.var(0, unbiased=False) + 1e-5)
        for mode in MODES:
            for split in (False, True):
                with ops.arithmetic(mode):
                    w = ops.presplit(c["dev"]["w"]) if split else c["dev"]["w"]
                    y, part, _, _ = run_form(ops, geom, c, form, w, colstats=True)
                    y0 = run_form(ops, geom, c, form, w)[0]
                assert part.shape == ((M + 63) // 64, Cout, 2)
                assert torch.equal(y, y0)
                st = ops.group_stats_from_colpart(part, M, Cout).double().cpu()
                em, er = float((st[:, 0] - mean).abs().max()), float(((st[:, 1] - rstd).abs() / rstd).max())
                print("conv colstats %s %s %s: mean abs err %.3g, rstd rel err %.3g" % (gid(geom), form, mode, em, er))
                close(st[:, 0], mean, 1e-4, (geom, form, mode, "mean"))
                close(st[:, 1], rstd, 1e-4, (geom, form, mode, "rstd"))


PLANS = [(64, 64, 1), (64, 128, 1), (128, 128, 1), (64, 64, 3), (128, 64, 1)]


@pytest.mark.parametrize("plan", PLANS, ids=lambda p: "%dx%dx%d" % p)
@pytest.mark.parametrize("geom", [R.ROW6, R.G9X15, R.CIN68], ids=gid)
def test_conv_forced_plans(ops, hooks, geom, plan):
    """every tile shape and a split K on the three geometries whose rows, columns and K do not fill a tile.  (64, 64, 3): K = 180 is cut
    into ranges of 128 - inside the seventh tap -, K = 612 into three of 256; K = 36 stays whole.  (128, 64, 1): bf16x6 only"""
    force, _ = hooks
    c = conv_case(geom)
    try:
        assert force(*plan) == 0
        for form in FORMS:
            for mode in (["bf16x6"] if plan == (128, 64, 1) else MODES):
                check_conv(ops, geom, c, form, mode, "plan %dx%dx%d" % plan)
    finally:
        force(0, 0, 0)
    report()


@pytest.mark.parametrize("direct", [0, 1, 2, -1], ids=["default", "2-row", "4-row", "off"])
@pytest.mark.parametrize("geom", R.DIRECT_GEOMS, ids=gid)
def test_conv_direct_kernel_smallest_maps(ops, hooks, geom, direct):
    """4 x 64 and 8 x 64 pixels x 16 -> 64 channels in bf16x6: default dispatch, the direct 3 x 3 kernel forced with 2-row and with 4-row
    tiles, and switched off (the hook of test_direct_3x3_convolution_bf16x6)"""
    _, hook = hooks
    c = conv_case(geom)
    try:
        assert hook(direct) == 0
        for form in FORMS:
            check_conv(ops, geom, c, form, "bf16x6", "direct=%d" % direct)
    finally:
        hook(0)
    report()


@pytest.mark.parametrize("mode", ["bf16x3", "bf16x6"])
@pytest.mark.parametrize("geom", R.NORM_GEOMS, ids=gid)
def test_conv_pending_norm(ops, geom, mode):
    """conv -> pending InstanceNorm + ReLU (ops.Normed over the first convolution's ColStats) -> conv with pre-split weights.  One frame of
    63 pixels and two of 128 fuse the normalisation into the operand loader; three frames of 63 pixels - statistics slabs that straddle
    frames - take the materialising fallback.  The reference starts from the kernel's own y1.  Bound: the 3e-4 (absolute + relative) of
    test_conv2d_normalising_loader."""
    H, W, Cin, Cout, ks, stride, pad, frames = geom
    g = torch.Generator().manual_seed(H * W + frames)
    x = torch.randn(frames * H * W, Cin, generator=g)
    wa = torch.randn(Cin, 9 * Cin, generator=g) / (9 * Cin) ** 0.5
    wb = torch.randn(Cout, 9 * Cin, generator=g) / (9 * Cin) ** 0.5
    with ops.arithmetic(mode):
        y1, p1, _, _ = ops.conv2d_nhwc(G(x), H, W, ops.presplit(G(wa)), 3, 1, 1, colstats=True, frames=frames)
        nm = ops.Normed(y1, ops.ColStats(p1, y1.shape[0], Cin, frames), slope=0.0)
        fuses = nm.fusable(frames == 1 or (H * W) % 128 == 0)
        assert fuses == (geom != R.NORM_GEOMS[1]), "which path this geometry takes"
        y2, Ho, Wo = ops.conv2d_nhwc(nm, H, W, ops.presplit(G(wb)), 3, 1, 1, frames=frames)
        y2m = ops.conv2d_nhwc(nm.materialize(), H, W, ops.presplit(G(wb)), 3, 1, 1, frames=frames)[0]
    assert (Ho, Wo) == (H, W)
    # the first convolution by the bounds of every other case (the second one's reference starts from y1: it cannot see an error in it)
    ref1, scale1 = R.conv2d_nhwc_ref(x, H, W, wa, 3, 1, 1, frames=frames), R.abs_scale(x, H, W, wa, 3, 1, 1, frames)
    base1 = scaled_err(R.to_rows(F.conv2d(R.to_nchw(x, H, W, frames), R.weight_oihw(wa, 3), None, 1, 1)), ref1, scale1)
    err1 = scaled_err(y1, ref1, scale1)
    print("conv pending norm %s %s: first convolution %.3g | bound %.3g (torch f32 %.3g)" % (gid(geom), mode, err1, bound(mode, base1), base1))
    note(mode, err1), note("torch f32", base1)
    assert err1 < bound(mode, base1), (geom, mode, "first convolution", err1)
    ref = R.conv2d_nhwc_ref(R.instance_norm_relu_ref(y1, frames), H, W, wb, 3, 1, 1, frames=frames)
    print("conv pending norm %s %s (%s): max abs err %.3g, materialised %.3g" % (gid(geom), mode, "fused" if fuses else "fallback",
                                                                                 float((y2.double().cpu() - ref).abs().max()), float((y2m.double().cpu() - ref).abs().max())))
    close(y2, ref, 3e-4, (geom, mode))
    close(y2m, ref, 3e-4, (geom, mode, "materialised"))
    assert torch.equal(y2, y2m), "the loader's normalisation and the apply kernel's give other bits"


def test_conv_refusals(ops, CofiError):
    """each call is refused on the host (conv_entry's argument checks) and leaves its output untouched.  Every operand is as large as the
    call's shapes ask for, or the head of a larger buffer: a missing check would show as a failed assertion, not as a stray access"""
    H, W, Cout = 5, 6, 12
    M = H * W
    room = torch.randn(8192, device=DEV)

    def x_of(Cin):
        return room[:M * Cin].reshape(M, Cin)

    def w_of(K):
        return room[4096:4096 + Cout * K].reshape(Cout, K)

    wide = room[2048:2048 + M * 16].reshape(M, 16)
    # what -> (call, rows of its output): ks = 2 / pad 1 gives 6 x 7 pixels, everything else 5 x 6
    cases = {
        "Cin = 6": (lambda o: ops.conv2d_nhwc(x_of(6), H, W, w_of(54), 3, 1, 1, out=o), M),
        "ks = 2": (lambda o: ops.conv2d_nhwc(x_of(8), H, W, w_of(32), 2, 1, 1, out=o), 42),
        "ks = 5": (lambda o: ops.conv2d_nhwc(x_of(8), H, W, w_of(200), 5, 1, 2, out=o), M),
        "x at a column offset of 2": (lambda o: ops.conv2d_nhwc(wide[:, 2:10], H, W, w_of(72), 3, 1, 1, out=o), M),
        "act_col0 > Cout": (lambda o: ops.conv2d_nhwc(x_of(8), H, W, w_of(72), 3, 1, 1, act=ops.ACT_RELU, act_col0=Cout + 1, out=o), M),
        "stat_width = 3": (lambda o: ops.conv2d_nhwc(x_of(8), H, W, w_of(72), 3, 1, 1, colstats=True, stat_width=3, out=o), M),
    }
    for mode in MODES:
        for what, (call, rows) in cases.items():
            out = torch.full((64, Cout), SENT, device=DEV)
            with ops.arithmetic(mode), pytest.raises(CofiError):
                call(out[:rows])
            assert bool((out == SENT).all()), (what, mode, "a refused call wrote to its output")
        # and the same operands, in order, are accepted
        with ops.arithmetic(mode):
            y = ops.conv2d_nhwc(x_of(8), H, W, w_of(72), 3, 1, 1)[0]
        assert bool(torch.isfinite(y).all())


# ====================================================================================================================== max-pool
def pool_input(H, W, C, frames):
    """all <= -1: a padding value of 0 would win every border maximum"""
    g = torch.Generator().manual_seed(H * 31 + W * 7 + C)
    return -(torch.rand(frames * H * W, C, generator=g) + 1.0)


@pytest.mark.parametrize("H,W,C,frames", R.POOL_SHAPES)
def test_maxpool_edge_maps(ops, H, W, C, frames):
    x = pool_input(H, W, C, frames)
    if (H, W) == (5, 9):
        x[::7] = -float("inf")                  # whole pixels of -inf, and a window of nothing else
        x[:2 * W + 3] = -float("inf")
    y, Ho, Wo = ops.maxpool3x3s2_nhwc(G(x), H, W, frames)
    want = F.max_pool2d(R.to_nchw(x, H, W, frames), 3, 2, 1)
    assert (Ho, Wo) == tuple(want.shape[2:]) and y.shape == (frames * Ho * Wo, C)
    assert torch.equal(y.cpu(), R.to_rows(want)), "not bit-equal to max_pool2d"
    assert torch.equal(y.cpu().double(), R.maxpool3x3s2_ref(x, H, W, frames)[0])
    assert bool((y <= -1.0).all())
    for f in range(frames):
        one = ops.maxpool3x3s2_nhwc(G(x[f * H * W:(f + 1) * H * W].contiguous()), H, W)[0]
        assert torch.equal(y[f * Ho * Wo:(f + 1) * Ho * Wo], one), "frame %d of the stacked call differs from the single-frame call" % f


def test_maxpool_grid_stride_loop(ops):
    """511 x 513 x 128 channels: 256 x 257 output pixels x 32 float4 = 2,105,344 work items, more than the 8192 x 256 threads of the capped
    grid.  Reference: max_pool2d in float64 on the GPU"""
    H, W, C = 511, 513, 128
    Ho, Wo = 256, 257
    assert Ho * Wo * C // 4 > 8192 * 256 >= (Ho * Wo - Wo) * C // 4
    x = -(torch.rand((H * W, C), device=DEV, generator=torch.Generator(device=DEV).manual_seed(1)) + 1.0)
    y, ho, wo = ops.maxpool3x3s2_nhwc(x, H, W)
    assert (ho, wo) == (Ho, Wo)
    want = F.max_pool2d(x.double().reshape(1, H, W, C).permute(0, 3, 1, 2), 3, 2, 1)[0].permute(1, 2, 0).reshape(Ho * Wo, C)
    first = 8192 * 256 // (C // 4)
    bad = (y.double() != want).any(1).nonzero()
    assert bad.numel() == 0, "first wrong row %d; the second sweep of the grid starts at row %d" % (int(bad[0]), first)


# ====================================================================================================================== up-sampling
@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("h,w,C1,C2,frames", R.UP_SHAPES)
def test_upsample_edge_maps(ops, h, w, C1, C2, frames, strided):
    g = torch.Generator().manual_seed(h * 31 + w * 7 + C1)
    low, skip = torch.randn(frames * h * w, C1, generator=g), torch.randn(frames * 4 * h * w, C2, generator=g)
    put = (lambda t: wide_of(t)[0]) if strided else G
    out = ops.upsample2x_cat_nhwc(put(low), h, w, put(skip), frames)
    ref = R.upsample2x_cat_ref(low, h, w, skip, frames)
    assert out.shape == ref.shape
    close(out[:, :C1], ref[:, :C1], 1e-6, (h, w, C1, C2, frames, strided))
    assert torch.equal(out[:, C1:].cpu(), skip), "the skip half is a copy"
    # across frames: the neighbouring frames hold 1e6, so a border pixel that reads another frame's row cannot hide
    P = h * w
    for f in range(frames if frames > 1 else 0):
        lone = torch.full_like(low, 1e6)
        lone[f * P:(f + 1) * P] = low[f * P:(f + 1) * P]
        o = ops.upsample2x_cat_nhwc(put(lone), h, w, put(skip), frames)
        close(o[f * 4 * P:(f + 1) * 4 * P, :C1], R.upsample2x_cat_ref(low[f * P:(f + 1) * P], h, w, skip[f * 4 * P:(f + 1) * 4 * P])[:, :C1], 1e-6,
              (h, w, frames, strided, "frame %d reads a neighbour" % f))
        assert torch.equal(o[f * 4 * P:(f + 1) * 4 * P], out[f * 4 * P:(f + 1) * 4 * P])


def test_upsample_grid_stride_loop(ops):
    """128 x 129 x (64 + 64) channels: 66048 output pixels x 32 float4 = 2,113,536 work items > 8192 x 256.  Reference: F.interpolate in
    float64 on the GPU"""
    h, w, C1, C2 = 128, 129, 64, 64
    assert 4 * h * w * (C1 + C2) // 4 > 8192 * 256 >= 4 * h * (w - 1) * (C1 + C2) // 4
    g = torch.Generator(device=DEV).manual_seed(2)
    low, skip = torch.randn((h * w, C1), device=DEV, generator=g), torch.randn((4 * h * w, C2), device=DEV, generator=g)
    out = ops.upsample2x_cat_nhwc(low, h, w, skip)
    up = F.interpolate(low.double().t().reshape(1, C1, h, w), scale_factor=2, mode="bilinear", align_corners=False).reshape(C1, 4 * h * w).t()
    first = 8192 * 256 // ((C1 + C2) // 4)
    err = (out[:, :C1].double() - up).abs() - 1e-6 * up.abs()
    bad = ((err > 1e-6).any(1) | (out[:, C1:] != skip).any(1)).nonzero()
    assert bad.numel() == 0, "first wrong row %d; the second sweep of the grid starts at row %d" % (int(bad[0]), first)


# ====================================================================================================================== im2col of the stem
@pytest.mark.parametrize("kpad", R.STEM_KPADS)
@pytest.mark.parametrize("frames,H,W", R.STEM_SHAPES)
def test_im2col_stem_edge_maps(ops, frames, H, W, kpad):
    img = torch.randn(frames, 3, H, W, generator=torch.Generator().manual_seed(H * 31 + W)) + 3.0      # no zeros of its own
    col, Ho, Wo = ops.im2col_stem(G(img), kpad)
    ref, ho, wo = R.im2col_stem_ref(img, kpad)
    assert (Ho, Wo) == (ho, wo) and col.shape == ref.shape
    assert torch.equal(col.double().cpu(), ref), "not bit-equal to the reference"
    assert torch.equal(col[:, 147:].cpu(), torch.zeros(frames * Ho * Wo, kpad - 147))
    for f in range(frames):
        one = ops.im2col_stem(G(img[f]), kpad)[0]
        assert torch.equal(col[f * Ho * Wo:(f + 1) * Ho * Wo], one)


def test_im2col_stem_grid_stride_loop(ops):
    """227 x 229 image: 114 x 115 output pixels x 160 columns = 2,097,600 elements, more than the 8192 x 256 threads of the capped grid.
    Reference: F.unfold in float64 on the GPU"""
    H, W, kpad = 227, 229, 160
    Ho, Wo = 114, 115
    assert Ho * Wo * kpad > 8192 * 256
    img = torch.randn((1, 3, H, W), device=DEV, generator=torch.Generator(device=DEV).manual_seed(3)) + 3.0
    col, ho, wo = ops.im2col_stem(img, kpad)
    assert (ho, wo) == (Ho, Wo)
    u = F.unfold(img.double(), 7, padding=3, stride=2).reshape(3, 49, Ho * Wo).permute(2, 1, 0).reshape(Ho * Wo, 147)
    want = torch.cat([u, torch.zeros((Ho * Wo, kpad - 147), dtype=torch.float64, device=DEV)], 1)
    first = 8192 * 256 // kpad
    bad = (col.double() != want).any(1).nonzero()
    assert bad.numel() == 0, "first wrong row %d; the second sweep of the grid starts inside row %d" % (int(bad[0]), first)


# ====================================================================================================================== wrapper checks
# No operand below is short: a surplus of rows (fewer frames asked for than the map holds included), or a column slice of a wider buffer
# whose dense span lies inside the allocation - even an unchecked launch would stay inside live memory, and shows as a failed assertion.
def test_glue_wrappers_refuse_maps_the_kernels_would_misread(ops, CofiError):
    H, W, C = 4, 6, 8
    buf = torch.full((H * W + 5, 2 * C), -2.0, device=DEV)
    bad_pool = {
        "a surplus of rows": (buf[:, :C].contiguous(), 1),
        "a column slice (leading dimension 16)": (buf[:H * W, :C], 1),
        "a column slice at an offset": (buf[:H * W, 4:4 + C], 1),
        "two frames asked of three": (torch.full((3 * H * W, C), -2.0, device=DEV), 2),
        "float64": (buf[:H * W, :C].contiguous().double(), 1),
        "C = 6": (buf[:H * W].reshape(-1)[:H * W * 6].reshape(H * W, 6), 1),
        "three dimensions": (buf[:H * W, :C].contiguous().reshape(H, W, C), 1),
    }
    for what, (x, frames) in bad_pool.items():
        with pytest.raises(CofiError):
            ops.maxpool3x3s2_nhwc(x, H, W, frames)
    y, Ho, Wo = ops.maxpool3x3s2_nhwc(buf[:H * W, :C].contiguous(), H, W)
    assert (Ho, Wo) == (2, 3) and bool((y == -2.0).all())

    h, w, C1, C2 = 2, 3, 8, 4
    lowb, skipb = torch.ones((h * w + 3, C1), device=DEV), torch.ones((4 * h * w + 3, C2), device=DEV)
    low, skip = lowb[:h * w], skipb[:4 * h * w]
    bad_up = {
        "low with a surplus of rows": (lowb, skip, 1),
        "skip with a surplus of rows": (low, skipb, 1),
        "low with one more row": (lowb[:h * w + 1], skip, 1),
        "two frames asked of three": (torch.ones((3 * h * w, C1), device=DEV), torch.ones((12 * h * w, C2), device=DEV), 2),
        "low in float64": (low.double(), skip, 1),
    }
    for what, (lo, sk, frames) in bad_up.items():
        with pytest.raises(CofiError):
            ops.upsample2x_cat_nhwc(lo, h, w, sk, frames)
    out = ops.upsample2x_cat_nhwc(low, h, w, skip)
    assert out.shape == (4 * h * w, C1 + C2) and bool((out == 1.0).all())


def test_pending_norm_over_straddling_slabs_materialises_from_the_map(ops):
    """ops.Normed.materialize on a stacked batch whose 64-row statistics slabs straddle frames (3 x 63 rows): the partials cannot give
    per-frame statistics, so they are taken from the map itself - against the float64 InstanceNorm + ReLU of each frame"""
    frames, P, C = 3, 63, 8
    x = torch.randn(frames * P, C, generator=torch.Generator().manual_seed(5)) * 2 + 0.5
    with ops.arithmetic("f32"):
        y, part = ops.gemm_colstats(G(x), torch.eye(C, device=DEV))
    assert torch.equal(y.cpu(), x)
    st = ops.ColStats(part, frames * P, C, frames)
    assert not st.fusable()
    close(ops.Normed(y, st, slope=0.0).materialize(), R.instance_norm_relu_ref(x, frames), 2e-5)
