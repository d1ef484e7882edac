"""Plain float64 references of the operators of csrc/norm.hip (GroupNorm statistics and apply, LayerNorm with its activation and residual
forms, column / row norms, column means, the sine position embedding), shared by tests/test_norm_refs_cpu.py - which checks each of them
against torch.nn.functional or the CPU oracle - and tests/test_norm_edges_gpu.py - which judges the HIP kernels by them.  Also the fp32
emulation of the order in which the apply kernel sums a row for its row_pos flag.  Everything takes CPU or device tensors of any float
type and returns float64 on the CPU."""
import math

import torch


def _d(t):
    return None if t is None else t.detach().double().cpu()


def leaky(v, slope):
    return torch.where(v >= 0, v, v * slope)


def group_stats(x, groups, eps=1e-5, frames=1):
    """x (frames * Mf, C) -> (mean, rstd), each (frames, groups): biased variance over the Mf rows and C / groups channels of a group."""
    x = _d(x)
    M, C = x.shape
    v = x.reshape(frames, M // frames, groups, C // groups)
    mean = v.mean((1, 3))
    var = ((v - mean[:, None, :, None]) ** 2).mean((1, 3))
    return mean, 1.0 / torch.sqrt(var + eps)


def _stat_pair(stats, frames):
    """(mean, rstd) tuple or a (groups, 2) / (frames, groups, 2) tensor -> two (frames, groups) float64 tensors"""
    if isinstance(stats, (tuple, list)):
        mean, rstd = (_d(s).reshape(frames, -1) for s in stats)
    else:
        s = _d(stats).reshape(frames, -1, 2)
        mean, rstd = s[..., 0], s[..., 1]
    return mean, rstd


def _normalise(x, stats, gamma, beta, frames):
    M, C = x.shape
    mean, rstd = _stat_pair(stats, frames)
    cpg = C // mean.shape[1]
    mean, rstd = (s.repeat_interleave(cpg, 1)[:, None, :] for s in (mean, rstd))   # (frames, 1, C)
    y = (x.reshape(frames, M // frames, C) - mean) * rstd
    if gamma is not None:
        y = y * _d(gamma) + _d(beta)
    return y.reshape(M, C)


def group_norm_apply(x, stats, gamma=None, beta=None, slope=1.0, res=None, res_stats=None, res_gamma=None, res_beta=None, frames=1):
    """leaky((x - mean) rstd gamma + beta + r, slope) with r = res, or the residual normalised by its own statistics (and affine pair)."""
    y = _normalise(_d(x), stats, gamma, beta, frames)
    if res is not None:
        y = y + (_d(res) if res_stats is None else _normalise(_d(res), res_stats, res_gamma, res_beta, frames))
    return leaky(y, slope)


def layer_norm_act(x, gamma, beta, eps=1e-5, slope=1.0, res=None, res_first=True):
    """leaky(LN(x) gamma + beta + (res if res_first), slope) + (res if not res_first); LN over each row, biased variance."""
    x, r = _d(x), _d(res)
    mean = x.mean(1, keepdim=True)
    var = ((x - mean) ** 2).mean(1, keepdim=True)
    y = (x - mean) / torch.sqrt(var + eps) * _d(gamma) + _d(beta)
    if r is not None and res_first:
        y = y + r
    y = leaky(y, slope)
    if r is not None and not res_first:
        y = y + r
    return y


def col_inv_norm(x, eps=1e-12):
    return 1.0 / torch.sqrt((_d(x) ** 2).sum(0)).clamp_min(eps)


def l2norm_rows(x, eps=1e-12):
    x = _d(x)
    return x / torch.sqrt((x ** 2).sum(1, keepdim=True)).clamp_min(eps)


def col_mean(x, frames=1):
    x = _d(x)
    return x.reshape(frames, x.shape[0] // frames, x.shape[1]).mean(1)


def pos_sine(coords, d_model=128):
    """position_encoding.py:39-50: channel d F + i = sin / cos (even / odd i) of coords[:, d] 2 pi / dim_t[i], zero beyond n_dim F.  dim_t
    is the fp32 table the kernel is handed (ops.sine_frequencies), widened; the angle and the functions are float64.  -> (emb, |angle| max)"""
    from cofii2p_amd.ops import sine_frequencies

    c = _d(coords)
    T, n_dim = c.shape
    dim_t = torch.from_numpy(sine_frequencies(n_dim, d_model)).double()
    F = dim_t.numel()
    ang = c[:, :, None] * (2.0 * math.pi) / dim_t           # (T, n_dim, F)
    even = (torch.arange(F) % 2 == 0)
    emb = torch.where(even, torch.sin(ang), torch.cos(ang)).reshape(T, n_dim * F)
    out = torch.zeros((T, d_model), dtype=torch.float64)
    out[:, :n_dim * F] = emb
    return out, float(ang.abs().max())


def row_sum_tree_f32(y):
    """The fp32 row sum of gn_apply_rows (csrc/norm.hip), bit for bit: per float4 chunk (v0 + v1) + (v2 + v3), then a balanced pairwise tree
    over the C / 4 chunks (a power of two) - what the xor butterfly leaves in the row's first lane.  y (M, C) -> (M,) float32 on the CPU."""
    y = y.detach().float().cpu()
    M, C = y.shape
    n = C // 4
    assert C == 4 * n and n & (n - 1) == 0
    v = y.reshape(M, n, 4)
    t = (v[:, :, 0] + v[:, :, 1]) + (v[:, :, 2] + v[:, :, 3])
    while t.shape[1] > 1:
        t = t[:, 0::2] + t[:, 1::2]
    return t[:, 0]
