"""Plain float64 references of the image branch's operators on the kernels' own layouts (csrc/gemm.hip conv_entry, csrc/image.hip): maps
are pixel-major (frames * H * W, C) rows, convolution weights are (Cout, ks * ks * Cin) with column (dy * ks + dx) * Cin + c, the stem's
im2col matrix has column (dy * 7 + dx) * 3 + c.  Shared by tests/test_image_refs_cpu.py - which checks each of them against
torch.nn.functional and against scalar loops - and tests/test_image_edges_gpu.py - which judges the HIP kernels by them.  Everything takes
CPU or device tensors of any float type and returns float64 on the CPU; nothing here calls torch's convolution, pooling or interpolation."""
import torch

ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_LEAKY01 = 0, 1, 2, 3      # cofii2p_amd.ops.ACT_*


def _d(t):
    return None if t is None else t.detach().double().cpu()


def out_size(n, ks, stride, pad):
    return (n + 2 * pad - ks) // stride + 1


def to_rows(t):
    """(frames, C, H, W) -> (frames * H * W, C)"""
    F_, C, H, W = t.shape
    return t.permute(0, 2, 3, 1).reshape(F_ * H * W, C).contiguous()


def to_nchw(rows, H, W, frames=1):
    """(frames * H * W, C) -> (frames, C, H, W)"""
    return rows.reshape(frames, H, W, rows.shape[1]).permute(0, 3, 1, 2).contiguous()


def weight_rows(w):
    """OIHW -> (O, kh * kw * I), column (dy * kw + dx) * I + c"""
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1).contiguous()


def weight_oihw(wr, ks):
    """(O, ks * ks * I) -> OIHW"""
    O = wr.shape[0]
    return wr.reshape(O, ks, ks, wr.shape[1] // (ks * ks)).permute(0, 3, 1, 2).contiguous()


def _act(v, act):
    if act == ACT_RELU:
        return v.clamp_min(0.0)
    if act == ACT_SIGMOID:
        return 1.0 / (1.0 + torch.exp(-v))
    if act == ACT_LEAKY01:
        return torch.where(v >= 0, v, v * 0.1)
    return v


def _taps(x, H, W, ks, stride, pad, frames):
    """the ks * ks shifted, strided windows of the zero-padded map: yields (tap, (frames, Ho, Wo, Cin))"""
    Cin = x.shape[1]
    Ho, Wo = out_size(H, ks, stride, pad), out_size(W, ks, stride, pad)
    xp = torch.zeros((frames, H + 2 * pad, W + 2 * pad, Cin), dtype=torch.float64)
    xp[:, pad:pad + H, pad:pad + W] = x.reshape(frames, H, W, Cin)
    for dy in range(ks):
        for dx in range(ks):
            yield dy * ks + dx, xp[:, dy:dy + stride * (Ho - 1) + 1:stride, dx:dx + stride * (Wo - 1) + 1:stride]


def conv2d_nhwc_ref(x, H, W, w, ks, stride=1, pad=1, bias=None, res=None, act=ACT_NONE, act_col0=0, frames=1):
    """act_{columns >= act_col0}(conv(x, w) + bias + res): x (frames * H * W, Cin), w (Cout, ks * ks * Cin) -> (frames * Ho * Wo, Cout)"""
    x, w = _d(x), _d(w)
    Cin, Cout = x.shape[1], w.shape[0]
    assert x.shape[0] == frames * H * W and w.shape[1] == ks * ks * Cin
    Ho, Wo = out_size(H, ks, stride, pad), out_size(W, ks, stride, pad)
    y = torch.zeros((frames, Ho, Wo, Cout), dtype=torch.float64)
    for tap, win in _taps(x, H, W, ks, stride, pad, frames):
        y += win @ w[:, tap * Cin:(tap + 1) * Cin].t()
    y = y.reshape(frames * Ho * Wo, Cout)
    if bias is not None:
        y = y + _d(bias)
    if res is not None:
        y = y + _d(res)
    if act != ACT_NONE:
        y = torch.cat([y[:, :act_col0], _act(y[:, act_col0:], act)], 1)
    return y


def abs_scale(x, H, W, w, ks, stride=1, pad=1, frames=1):
    """the convolution of |x| with |w|: the sum of the |products| behind every output, the error scale of a contraction"""
    return conv2d_nhwc_ref(_d(x).abs(), H, W, _d(w).abs(), ks, stride, pad, frames=frames)


def maxpool3x3s2_ref(x, H, W, frames=1):
    """3 x 3 / stride 2 / pad 1 maximum over the pixels INSIDE the map: (frames * H * W, C) -> (frames * Ho * Wo, C), Ho, Wo"""
    x = _d(x)
    C = x.shape[1]
    Ho, Wo = out_size(H, 3, 2, 1), out_size(W, 3, 2, 1)
    xp = torch.full((frames, H + 2, W + 2, C), -float("inf"), dtype=torch.float64)
    xp[:, 1:1 + H, 1:1 + W] = x.reshape(frames, H, W, C)
    y = torch.full((frames, Ho, Wo, C), -float("inf"), dtype=torch.float64)
    for dy in range(3):
        for dx in range(3):
            y = torch.maximum(y, xp[:, dy:dy + 2 * (Ho - 1) + 1:2, dx:dx + 2 * (Wo - 1) + 1:2])
    return y.reshape(frames * Ho * Wo, C), Ho, Wo


def _bilinear_axis(n):
    """x2, align_corners=False, along an axis of n source pixels: (i0, i1, weight of i1) per output index"""
    o = torch.arange(2 * n, dtype=torch.float64)
    s = (0.5 * (o + 0.5) - 0.5).clamp_min(0.0)
    i0 = s.floor().long()
    i1 = torch.where(i0 < n - 1, i0 + 1, i0)
    return i0, i1, s - i0.double()


def upsample2x_cat_ref(low, h, w, skip, frames=1):
    """[bilinear x2 of low (frames * h * w, C1) | skip (frames * 4 h w, C2)] -> (frames * 4 h w, C1 + C2)"""
    low, skip = _d(low), _d(skip)
    C1 = low.shape[1]
    v = low.reshape(frames, h, w, C1)
    y0, y1, ly = _bilinear_axis(h)
    x0, x1, lx = _bilinear_axis(w)
    ly, lx = ly[None, :, None, None], lx[None, None, :, None]
    top = v[:, y0][:, :, x0] * (1 - lx) + v[:, y0][:, :, x1] * lx
    bot = v[:, y1][:, :, x0] * (1 - lx) + v[:, y1][:, :, x1] * lx
    up = (top * (1 - ly) + bot * ly).reshape(frames * 4 * h * w, C1)
    assert skip.shape[0] == up.shape[0]
    return torch.cat([up, skip], 1)


def im2col_stem_ref(img, kpad=160):
    """7 x 7 / stride 2 / pad 3 patches of img (frames, 3, H, W): -> (frames * Ho * Wo, kpad), Ho, Wo; column (dy * 7 + dx) * 3 + c,
    columns 147 ... kpad - 1 zero"""
    img = _d(img)
    if img.dim() == 3:
        img = img[None]
    frames, _, H, W = img.shape
    Ho, Wo = out_size(H, 7, 2, 3), out_size(W, 7, 2, 3)
    out = torch.zeros((frames, Ho, Wo, kpad), dtype=torch.float64)
    for tap, win in _taps(to_rows(img), H, W, 7, 2, 3, frames):
        out[..., 3 * tap:3 * tap + 3] = win
    return out.reshape(frames * Ho * Wo, kpad), Ho, Wo


def instance_norm_relu_ref(y, frames=1, eps=1e-5):
    """relu((y - mean) / sqrt(var + eps)) per frame and channel (biased variance): the pending normalisation ops.Normed(y, ColStats(...,
    groups = C), slope = 0) stands for"""
    y = _d(y)
    v = y.reshape(frames, y.shape[0] // frames, y.shape[1])
    mean = v.mean(1, keepdim=True)
    var = ((v - mean) ** 2).mean(1, keepdim=True)
    return ((v - mean) / torch.sqrt(var + eps)).clamp_min(0.0).reshape(y.shape)


# ------------------------------------------------------------------------------------------ the edge geometries both test modules use
# (H, W, Cin, Cout, ks, stride, pad, frames)
CONV_GEOMS = [
    (1, 1, 4, 4, 3, 1, 1, 1),         # one pixel: eight of nine taps are padding
    (1, 6, 8, 4, 3, 1, 1, 1),         # one row
    (5, 1, 4, 8, 3, 1, 1, 1),         # one column
    (3, 3, 8, 8, 3, 1, 0, 1),         # kernel as large as the map: one output pixel
    (6, 6, 4, 4, 3, 2, 0, 2),         # the stride never reads the last row and column; two frames
    (7, 9, 4, 16, 3, 2, 1, 3),        # odd sizes, stride 2; 20 output pixels per frame: three frames in one row tile; K = 36 < one K tile
    (7, 9, 12, 68, 1, 2, 0, 2),       # 1 x 1 stride 2; Cout = 68: a column-tile tail that is no multiple of 64
    (9, 15, 20, 130, 3, 1, 1, 1),     # M = 135, N = 130: partial last row and column tiles; K = 180: two K tiles and a tail
    (5, 13, 68, 32, 3, 1, 1, 5),      # Cin = 68: every 64-deep K tile crosses a tap; five frames of 65 rows
]
ROW6, G9X15, CIN68 = CONV_GEOMS[5], CONV_GEOMS[7], CONV_GEOMS[8]
DIRECT_GEOMS = [(4, 64, 16, 64, 3, 1, 1, 1), (8, 64, 16, 64, 3, 1, 1, 3)]      # the smallest maps of the direct 3 x 3 kernel
NORM_GEOMS = [(7, 9, 8, 16, 3, 1, 1, 1), (7, 9, 8, 16, 3, 1, 1, 3), (16, 8, 8, 16, 3, 1, 1, 2)]      # pending-norm chains
POOL_SHAPES = [(1, 1, 4, 1), (1, 7, 4, 1), (7, 1, 8, 2), (5, 9, 12, 3), (6, 8, 68, 2)]              # (H, W, C, frames)
UP_SHAPES = [(1, 1, 4, 4, 1), (1, 5, 4, 8, 1), (3, 1, 8, 4, 2), (2, 3, 12, 20, 3)]                  # (h, w, C1, C2, frames)
STEM_SHAPES = [(1, 1, 1), (1, 7, 7), (2, 5, 9), (3, 8, 6)]                                           # (frames, H, W)
STEM_KPADS = [148, 160]


def conv_case(geom, seed=0):
    """the inputs of one convolution geometry, fp32 on the CPU: x, w (scaled by K^-1/2), bias, residual"""
    H, W, Cin, Cout, ks, stride, pad, frames = geom
    g = torch.Generator().manual_seed(1000 * seed + 131 * H + 17 * W + Cin + Cout)
    K = ks * ks * Cin
    Ho, Wo = out_size(H, ks, stride, pad), out_size(W, ks, stride, pad)
    x = torch.randn(frames * H * W, Cin, generator=g)
    w = torch.randn(Cout, K, generator=g) / K ** 0.5
    bias = torch.randn(Cout, generator=g)
    res = torch.randn(frames * Ho * Wo, Cout, generator=g)
    return x, w, bias, res
