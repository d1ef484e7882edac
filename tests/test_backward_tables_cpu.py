"""CPU side of the backward-operator tests: the transposed index table (autograd.TransposedTable) against a plain numpy CSR build,
out-of-range entries included - the only place they appear; no kernel is ever handed one - and the three float64 references of
tests/backward_refs.py against torch.autograd on tie-free data, so that a failure of tests/test_backward_edges_gpu.py points at the
kernel and not at the reference."""
import math

import numpy as np
import pytest
import torch

import backward_refs as R


def _csr_numpy(flat, N):
    """lists[j] = ascending positions p with flat[p] == j, for 0 <= j < N; everything else is dropped"""
    lists = [[] for _ in range(N)]
    for p, j in enumerate(flat.tolist()):
        if 0 <= j < N:
            lists[j].append(p)
    offsets = np.zeros(N + 1, np.int64)
    offsets[1:] = np.cumsum([len(l) for l in lists])
    pairs = np.array([p for l in lists for p in l], np.int64)
    return offsets, pairs


@pytest.mark.parametrize("two_d", [True, False])
def test_transposed_table_against_numpy_csr(two_d):
    from cofii2p_amd.autograd import TransposedTable

    g = np.random.default_rng(5)
    N, M, H = 40, 60, 12
    idx = g.integers(2, N, (M, H))          # rows 0 and 1 are placed by hand
    flat = idx.reshape(-1)
    where = g.permutation(M * H)
    flat[where[:200]] = 1                   # support row 1: listed 200 times; row 0: never
    flat[where[200:230]] = N                # shadow entries
    flat[where[230:245]] = -1
    flat[where[245:260]] = N + 3
    assert (flat == 0).sum() == 0 and (flat == 1).sum() == 200
    t_idx = torch.from_numpy(idx.astype(np.int32)) if two_d else torch.from_numpy(flat.astype(np.int32).copy())
    t = TransposedTable(t_idx, N)
    assert (t.N, t.M, t.H) == ((N, M, H) if two_d else (N, M * H, 1))
    assert t.pairs.dtype == torch.int32 and t.offsets.dtype == torch.int32
    off, pairs = t.offsets.numpy().astype(np.int64), t.pairs.numpy().astype(np.int64)
    ref_off, ref_pairs = _csr_numpy(flat, N)
    in_range = int(((flat >= 0) & (flat < N)).sum())
    assert off.shape == (N + 1,) and (np.diff(off) >= 0).all()
    assert off[N] - off[0] == in_range == ref_off[N]
    assert off[0] == (flat < 0).sum()       # negative keys sort in front of list 0 and are never visited
    assert off[1] - off[0] == 0 and off[2] - off[1] == 200
    np.testing.assert_array_equal(off - off[0], ref_off)
    np.testing.assert_array_equal(pairs[off[0]:off[N]], ref_pairs)
    for j in range(N):
        lst = pairs[off[j]:off[j + 1]]
        assert (np.diff(lst) > 0).all(), j                      # ascending inside a list: the fixed summation order
        assert (flat[lst] == j).all(), j                        # every pair maps back to its support row
        if two_d:
            assert (idx[lst // H, lst % H] == j).all(), j


def test_fan_in_table_has_the_prescribed_lists():
    g = np.random.default_rng(1)
    idx = R.fan_in_table(g, 300, 180, 24, [0, 64, 65, 128, 200])
    cnt = np.bincount(idx.reshape(-1), minlength=301)
    assert list(cnt[:5]) == [0, 64, 65, 128, 200] and cnt[300] > 0
    assert (idx[7, :5] == 4).all() and (idx[3] == 300).all()


def test_maxpool_reference_against_autograd_without_ties():
    g = torch.Generator().manual_seed(2)
    N, M, H, C = 50, 30, 9, 12
    x = torch.randn((N, C), generator=g, dtype=torch.float64)          # continuous data: no two equal values
    idx = torch.randint(0, N + 1, (M, H), generator=g)
    for m in range(M):                                                # no support row twice in a neighbourhood (that would be a tie)
        idx[m] = torch.randperm(N + 1, generator=g)[:H]
    idx[4] = N                                                        # H pad entries tie with each other - on the pad row, which takes no gradient
    dy = torch.randn((M, C), generator=g, dtype=torch.float64)
    xr = x.clone().requires_grad_()
    yr = torch.cat([xr, torch.zeros((1, C), dtype=torch.float64)], 0)[idx].max(1)[0]
    yr.backward(dy)
    y, dx, arg = R.maxpool_first_max_ref(x, idx, dy)
    assert torch.equal(y, yr.detach()) and torch.allclose(dx, xr.grad, rtol=0, atol=1e-14)
    assert int(arg.max()) < H and float(y[4].abs().max()) == 0.0


def test_maxpool_reference_takes_the_first_maximum():
    x = torch.tensor([[1.0, -1.0], [1.0, -2.0], [0.5, -3.0]], dtype=torch.float64)
    idx = torch.tensor([[2, 1, 0, 3], [3, 2, 2, 2]])
    dy = torch.tensor([[10.0, 20.0], [30.0, 40.0]], dtype=torch.float64)
    y, dx, arg = R.maxpool_first_max_ref(x, idx, dy)
    assert y.tolist() == [[1.0, 0.0], [0.5, 0.0]]
    assert arg.tolist() == [[1, 3], [1, 0]]                           # rows 1 and 0 tie at 1.0: h = 1 comes first; the pad row wins the negatives
    assert dx.tolist() == [[0.0, 0.0], [10.0, 0.0], [30.0, 0.0]]


def test_kpconv_reference_against_autograd():
    from cofii2p_amd.weights import kernel_point_table

    g = np.random.default_rng(3)
    N, M, H, C, sigma = 40, 25, 8, 6, 0.3
    s_pts, q_pts = torch.from_numpy(g.random((N, 3)) * 0.4), torch.from_numpy(g.random((M, 3)) * 0.4)
    idx = torch.from_numpy(g.integers(0, N + 1, (M, H)))
    kp = torch.from_numpy(kernel_point_table(15, 0.425 * sigma / 0.2)).double()
    feats, dagg = torch.from_numpy(g.standard_normal((N, C))), torch.from_numpy(g.standard_normal((M, 15 * C)))
    f = feats.clone().requires_grad_()
    out = []
    for m in range(M):                                                # kpconv.py:91-105 query by query, neighbour by neighbour
        acc = torch.zeros((15, C), dtype=torch.float64)
        for h in range(H):
            j = int(idx[m, h])
            if j == N:
                continue
            w = (1.0 - ((s_pts[j] - q_pts[m])[None] - kp).norm(dim=1) / sigma).clamp_min(0.0)
            acc = acc + w[:, None] * f[j][None]
        out.append(acc.reshape(-1))
    ref = torch.stack(out)
    ref.backward(dagg)
    agg, df, infl = R.kpconv_aggregate_ref(feats, q_pts, s_pts, idx, kp, sigma, dagg)
    assert infl.shape == (M, H, 15) and float((infl > 0).double().mean()) > 0.05
    assert torch.allclose(agg, ref.detach(), rtol=0, atol=1e-13) and torch.allclose(df, f.grad, rtol=0, atol=1e-13)


@pytest.mark.parametrize("L,S,H,qs", [(7, 5, 2, 0.7), (1, 1, 4, 0.7), (9, 40, 1, 12.0)])
def test_attention_reference_against_autograd(L, S, H, qs):
    D = 32
    g = torch.Generator().manual_seed(L + S)
    q = torch.randn((L, H * D), generator=g, dtype=torch.float64) * qs
    k, v, do = (torch.randn((n, H * D), generator=g, dtype=torch.float64) for n in (S, S, L))
    r = [t.clone().requires_grad_() for t in (q, k, v)]
    qh, kh, vh = (t.reshape(-1, H, D) for t in r)
    A = torch.softmax(torch.einsum("lhd,shd->hls", qh, kh) / math.sqrt(D), dim=-1)    # linear_attention.py:70-76
    orf = torch.einsum("hls,shd->lhd", A, vh).reshape(L, H * D)
    orf.backward(do)
    o, dq, dk, dv = R.attention_ref(q, k, v, do, H)
    for a, b in ((o, orf.detach()), (dq, r[0].grad), (dk, r[1].grad), (dv, r[2].grad)):
        assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))
