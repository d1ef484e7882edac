"""Plain float64 references of three operators of cofii2p_amd/autograd.py, forward AND gradient written out by hand (no autograd inside),
shared by tests/test_backward_tables_cpu.py - which checks each of them against torch.autograd on tie-free data - and
tests/test_backward_edges_gpu.py - which judges the HIP kernels by them.  Also the index tables with a prescribed fan-in per support
row that the list-walking adjoints (csrc/backward.hip: 64 pairs per round) are tested on."""
import math

import numpy as np
import torch


def maxpool_first_max_ref(x, idx, dy):
    """functional.py:53-66 with the tie rule spelled out: y[m, c] = max_h xp[idx[m, h], c], xp = x with a zero row appended (idx == N), and
    the gradient goes to the FIRST h attaining the maximum (np.argmax: first occurrence, documented) - nothing if that is the pad row.
    -> (y (M, C), dx (N, C), arg (M, C)) float64 / int64 torch tensors on the CPU."""
    xn, dyn = x.detach().double().cpu().numpy(), dy.detach().double().cpu().numpy()
    ii = idx.detach().cpu().numpy().astype(np.int64)
    N, C = xn.shape
    M, H = ii.shape
    xp = np.concatenate([xn, np.zeros((1, C))], 0)
    vals = xp[ii]                                   # (M, H, C)
    arg = np.argmax(vals, axis=1)                   # (M, C), first occurrence of the maximum
    y = np.take_along_axis(vals, arg[:, None, :], 1)[:, 0, :]
    rows = np.take_along_axis(ii, arg, 1)           # support row that wins (m, c)
    dx = np.zeros((N + 1, C))
    np.add.at(dx, (rows, np.broadcast_to(np.arange(C), (M, C))), dyn)
    return torch.from_numpy(y), torch.from_numpy(dx[:N].copy()), torch.from_numpy(arg)


def kpconv_influence(q_pts, s_pts, idx, kp, sigma):
    """(M, H, 15) float64 kernel-point influences max(1 - |(s[idx] - q) - kp| / sigma, 0) (kpconv.py:89-101); 0 for shadow entries."""
    q, s, k = q_pts.detach().double(), s_pts.detach().double(), kp.detach().double()
    N = s.shape[0]
    ii = idx.long()
    sp = torch.cat([s, torch.full((1, 3), 1e6, dtype=torch.float64, device=s.device)], 0)
    rel = sp[ii] - q[:, None, :]
    d = ((rel[:, :, None, :] - k[None, None]) ** 2).sum(-1).sqrt()
    infl = (1.0 - d / sigma).clamp_min(0.0)
    return infl * (ii < N)[:, :, None]


def kpconv_aggregate_ref(feats, q_pts, s_pts, idx, kp, sigma, dagg):
    """agg[m, k, c] = sum_h w(m, h, k) f[idx[m, h], c] and df[j, c] = sum_{idx[m, h] = j} sum_k w(m, h, k) dagg[m, k, c] in float64.
    -> (agg (M, 15 C), df (N, C), infl (M, H, 15))."""
    f, g = feats.detach().double(), dagg.detach().double()
    N, C = f.shape
    M, H = idx.shape
    infl = kpconv_influence(q_pts, s_pts, idx, kp, sigma)
    ii = idx.long()
    fp = torch.cat([f, torch.zeros((1, C), dtype=torch.float64, device=f.device)], 0)
    agg = torch.einsum("mhk,mhc->mkc", infl, fp[ii]).reshape(M, 15 * C)
    pair = torch.einsum("mhk,mkc->mhc", infl, g.reshape(M, 15, C))
    df = torch.zeros((N + 1, C), dtype=torch.float64, device=f.device).index_add_(0, ii.reshape(-1), pair.reshape(M * H, C))[:N]
    return agg, df, infl


def attention_ref(q, k, v, do, nhead):
    """softmax(q k^T / sqrt(D)) v per head (linear_attention.py:56-79) and its three gradients in float64:
    delta = rowsum(dO o O), dP = dO V^T, dS = P o (dP - delta) / sqrt(D), dQ = dS K, dK = dS^T Q, dV = P^T dO.  -> (o, dq, dk, dv)."""
    q, k, v, do = (t.detach().double() for t in (q, k, v, do))
    L, HD = q.shape
    S, D = k.shape[0], HD // nhead
    sc = 1.0 / math.sqrt(D)
    qh, kh, vh, doh = (t.reshape(-1, nhead, D).transpose(0, 1) for t in (q, k, v, do))     # (H, rows, D)
    s = qh @ kh.transpose(1, 2) * sc
    p = torch.exp(s - s.max(-1, keepdim=True)[0])
    p = p / p.sum(-1, keepdim=True)
    o = p @ vh
    dv = p.transpose(1, 2) @ doh
    dp = doh @ vh.transpose(1, 2)
    ds = p * (dp - (doh * o).sum(-1, keepdim=True)) * sc
    dq, dk = ds @ kh, ds.transpose(1, 2) @ qh
    back = lambda t, rows: t.transpose(0, 1).reshape(rows, HD)
    return back(o, L), back(dq, L), back(dk, S), back(dv, S)


def fan_in_table(g, N, M, H, counts, repeat=(4, 5), shadow=True, keep_free_of=()):
    """idx (M, H) int64 numpy with a prescribed number of listings for the first support rows: row j < len(counts) is listed exactly
    counts[j] times (0: never), the slots picked at random; rows >= len(counts) fill the rest at random.  repeat = (row, r): one query
    lists `row` in its first r slots (duplicates inside a neighbourhood, counted in counts[row]).  shadow: some entries == N as the
    reference pads short neighbourhoods (kpconv.py:89), one query with nothing else.  keep_free_of: queries that receive none of the
    counted rows (the caller overwrites them)."""
    nfix = len(counts)
    idx = g.integers(nfix, N, (M, H))
    free = np.ones((M, H), bool)
    if shadow:
        idx[::9, -2:] = N
        idx[3, :] = N
        free[::9, -2:] = False
        free[3, :] = False
    free[list(keep_free_of), :] = False
    left = list(counts)
    if repeat is not None:
        row, r = repeat
        qm = 7
        idx[qm, :r] = row
        free[qm, :r] = False
        left[row] -= r
    slots = np.flatnonzero(free.reshape(-1))
    slots = slots[g.permutation(slots.size)]
    flat = idx.reshape(-1)
    at = 0
    for j, n in enumerate(left):
        flat[slots[at:at + n]] = j
        at += n
    got = np.bincount(flat, minlength=N + 1)
    assert list(got[:nfix]) == list(counts), (got[:nfix], counts)
    return idx
