"""The float64 references of tests/image_refs.py, pinned independently of any kernel: each against torch.nn.functional in float64 at the
geometries tests/test_image_edges_gpu.py runs, the layout helpers against scalar Python loops on tiny cases, and every frame of a stacked
call against the single-frame call on its slice.  No GPU needed."""
import pytest
import torch
import torch.nn.functional as F

import image_refs as R

TOL = dict(rtol=1e-12, atol=1e-12)


def rn(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


@pytest.mark.parametrize("geom", R.CONV_GEOMS + R.DIRECT_GEOMS + R.NORM_GEOMS)
def test_convolution_reference(geom):
    H, W, Cin, Cout, ks, stride, pad, frames = geom
    x, w, bias, res = (t.double() for t in R.conv_case(geom))
    want = R.to_rows(F.conv2d(R.to_nchw(x, H, W, frames), R.weight_oihw(w, ks), None, stride, pad))
    Ho, Wo = R.out_size(H, ks, stride, pad), R.out_size(W, ks, stride, pad)
    assert want.shape == (frames * Ho * Wo, Cout)
    torch.testing.assert_close(R.conv2d_nhwc_ref(x, H, W, w, ks, stride, pad, frames=frames), want, **TOL)
    torch.testing.assert_close(R.conv2d_nhwc_ref(x, H, W, w, ks, stride, pad, bias=bias, frames=frames), want + bias, **TOL)
    torch.testing.assert_close(R.conv2d_nhwc_ref(x, H, W, w, ks, stride, pad, bias, res, R.ACT_RELU, frames=frames), torch.relu(want + bias + res), **TOL)
    c0 = Cout // 2
    half = R.conv2d_nhwc_ref(x, H, W, w, ks, stride, pad, bias, None, R.ACT_RELU, c0, frames)
    torch.testing.assert_close(half[:, :c0], (want + bias)[:, :c0], **TOL)
    torch.testing.assert_close(half[:, c0:], torch.relu(want + bias)[:, c0:], **TOL)
    torch.testing.assert_close(R.conv2d_nhwc_ref(x, H, W, w, ks, stride, pad, bias, act=R.ACT_LEAKY01, frames=frames), F.leaky_relu(want + bias, 0.1), **TOL)
    torch.testing.assert_close(R.conv2d_nhwc_ref(x, H, W, w, ks, stride, pad, bias, act=R.ACT_SIGMOID, frames=frames), torch.sigmoid(want + bias), **TOL)
    scale = R.abs_scale(x, H, W, w, ks, stride, pad, frames)
    torch.testing.assert_close(scale, R.to_rows(F.conv2d(R.to_nchw(x.abs(), H, W, frames), R.weight_oihw(w.abs(), ks), None, stride, pad)), **TOL)
    assert bool((scale >= want.abs() - 1e-12).all())
    # every frame of the stacked call is the single-frame call on its slice
    full = R.conv2d_nhwc_ref(x, H, W, w, ks, stride, pad, bias, res, R.ACT_RELU, frames=frames)
    for f in range(frames):
        one = R.conv2d_nhwc_ref(x[f * H * W:(f + 1) * H * W], H, W, w, ks, stride, pad, bias, res[f * Ho * Wo:(f + 1) * Ho * Wo], R.ACT_RELU)
        assert torch.equal(full[f * Ho * Wo:(f + 1) * Ho * Wo], one)


def test_abs_scale_is_the_gemm_scale_on_a_1x1_convolution():
    x, w = rn(35, 12, seed=1), rn(20, 12, seed=2)
    torch.testing.assert_close(R.abs_scale(x, 5, 7, w, 1, 1, 0), x.abs() @ w.abs().t(), **TOL)


@pytest.mark.parametrize("geom", [(3, 4, 2, 3, 3, 2, 1, 2), (2, 5, 3, 2, 1, 2, 0, 1)])
def test_convolution_reference_and_layout_helpers_by_scalar_loops(geom):
    H, W, Cin, Cout, ks, stride, pad, frames = geom
    x, w = rn(frames * H * W, Cin, seed=3), rn(Cout, ks * ks * Cin, seed=4)
    Ho, Wo = R.out_size(H, ks, stride, pad), R.out_size(W, ks, stride, pad)
    want = torch.zeros(frames * Ho * Wo, Cout, dtype=torch.float64)
    for f in range(frames):
        for yo in range(Ho):
            for xo in range(Wo):
                for n in range(Cout):
                    s = 0.0
                    for dy in range(ks):
                        for dx in range(ks):
                            yi, xi = yo * stride - pad + dy, xo * stride - pad + dx
                            if 0 <= yi < H and 0 <= xi < W:
                                for c in range(Cin):
                                    s += float(x[(f * H + yi) * W + xi, c]) * float(w[n, (dy * ks + dx) * Cin + c])
                    want[(f * Ho + yo) * Wo + xo, n] = s
    torch.testing.assert_close(R.conv2d_nhwc_ref(x, H, W, w, ks, stride, pad, frames=frames), want, **TOL)
    # layout helpers, element by element
    nchw, oihw = R.to_nchw(x, H, W, frames), R.weight_oihw(w, ks)
    assert nchw.shape == (frames, Cin, H, W) and oihw.shape == (Cout, Cin, ks, ks)
    for f in range(frames):
        for yi in range(H):
            for xi in range(W):
                for c in range(Cin):
                    assert nchw[f, c, yi, xi] == x[(f * H + yi) * W + xi, c]
    for n in range(Cout):
        for c in range(Cin):
            for dy in range(ks):
                for dx in range(ks):
                    assert oihw[n, c, dy, dx] == w[n, (dy * ks + dx) * Cin + c]
    assert torch.equal(R.to_rows(nchw), x) and torch.equal(R.weight_rows(oihw), w)


@pytest.mark.parametrize("H,W,C,frames", R.POOL_SHAPES + [(32, 48, 64, 1)])
def test_maxpool_reference(H, W, C, frames):
    x = -(torch.rand(frames * H * W, C, generator=torch.Generator().manual_seed(H + W), dtype=torch.float64) + 1.0)
    x[0, 0] = -float("inf")
    got, Ho, Wo = R.maxpool3x3s2_ref(x, H, W, frames)
    want = F.max_pool2d(R.to_nchw(x, H, W, frames), 3, 2, 1)
    assert (Ho, Wo) == tuple(want.shape[2:])
    assert torch.equal(got, R.to_rows(want))
    assert bool((got <= -1.0).all()), "padding must never win the maximum"
    for f in range(frames):
        assert torch.equal(got[f * Ho * Wo:(f + 1) * Ho * Wo], R.maxpool3x3s2_ref(x[f * H * W:(f + 1) * H * W], H, W)[0])


@pytest.mark.parametrize("h,w,C1,C2,frames", R.UP_SHAPES + [(20, 64, 8, 4, 1)])
def test_upsample_reference(h, w, C1, C2, frames):
    low, skip = rn(frames * h * w, C1, seed=5), rn(frames * 4 * h * w, C2, seed=6)
    got = R.upsample2x_cat_ref(low, h, w, skip, frames)
    up = F.interpolate(R.to_nchw(low, h, w, frames), scale_factor=2, mode="bilinear", align_corners=False)
    torch.testing.assert_close(got[:, :C1], R.to_rows(up), **TOL)
    assert torch.equal(got[:, C1:], skip)
    for f in range(frames):
        one = R.upsample2x_cat_ref(low[f * h * w:(f + 1) * h * w], h, w, skip[f * 4 * h * w:(f + 1) * 4 * h * w])
        assert torch.equal(got[f * 4 * h * w:(f + 1) * 4 * h * w], one)


@pytest.mark.parametrize("kpad", R.STEM_KPADS)
@pytest.mark.parametrize("frames,H,W", R.STEM_SHAPES + [(1, 64, 96)])
def test_im2col_stem_reference(frames, H, W, kpad):
    img = rn(frames, 3, H, W, seed=7)
    got, Ho, Wo = R.im2col_stem_ref(img, kpad)
    assert (Ho, Wo) == ((H - 1) // 2 + 1, (W - 1) // 2 + 1) and got.shape == (frames * Ho * Wo, kpad)
    # F.unfold: (frames, 3 * 49, Ho * Wo) with row c * 49 + dy * 7 + dx
    u = F.unfold(img, 7, padding=3, stride=2).reshape(frames, 3, 49, Ho * Wo).permute(0, 3, 2, 1).reshape(frames * Ho * Wo, 147)
    assert torch.equal(got[:, :147], u)
    assert torch.equal(got[:, 147:], torch.zeros(frames * Ho * Wo, kpad - 147, dtype=torch.float64))
    for f in range(frames):
        assert torch.equal(got[f * Ho * Wo:(f + 1) * Ho * Wo], R.im2col_stem_ref(img[f], kpad)[0])
    # the stem convolution is this matrix times the weight in the same column order
    w = rn(5, 3, 7, 7, seed=8)
    torch.testing.assert_close(got[:, :147] @ R.weight_rows(w).t(), R.to_rows(F.conv2d(img, w, None, 2, 3)), **TOL)


def test_im2col_stem_reference_by_a_scalar_loop():
    frames, H, W = 2, 3, 4
    img = rn(frames, 3, H, W, seed=9)
    got, Ho, Wo = R.im2col_stem_ref(img, 148)
    for f in range(frames):
        for yo in range(Ho):
            for xo in range(Wo):
                for k in range(148):
                    tap, c = divmod(k, 3)
                    dy, dx = divmod(tap, 7)
                    yi, xi = 2 * yo - 3 + dy, 2 * xo - 3 + dx
                    want = float(img[f, c, yi, xi]) if k < 147 and 0 <= yi < H and 0 <= xi < W else 0.0
                    assert float(got[(f * Ho + yo) * Wo + xo, k]) == want


def test_instance_norm_relu_reference():
    frames, P, C = 3, 63, 8
    y = rn(frames * P, C, seed=10) * 2 + 0.5
    want = torch.relu(F.instance_norm(R.to_nchw(y, 7, 9, frames), eps=1e-5))
    torch.testing.assert_close(R.instance_norm_relu_ref(y, frames), R.to_rows(want), rtol=1e-11, atol=1e-11)


def test_glue_wrappers_refuse_before_loading_anything():
    """the operand checks of ops.maxpool3x3s2_nhwc / ops.upsample2x_cat_nhwc are judged on tensor metadata: a CPU tensor never reaches a launch"""
    from cofii2p_amd import ops
    from cofii2p_amd._lib import CofiError

    with pytest.raises(CofiError):
        ops.maxpool3x3s2_nhwc(torch.zeros(6, 4), 2, 3)
    with pytest.raises(CofiError):
        ops.upsample2x_cat_nhwc(torch.zeros(6, 4), 2, 3, torch.zeros(24, 4))
