"""cofi_neighbor_maxpool_slice (the neighbour max-pool served from an LDS-resident source slice) against the gather kernel
cofi_neighbor_maxpool and the plain reference tests/maxpool_refs.py, bit for bit (torch.equal), every case twice; and how
ops.neighbor_maxpool routes between the two kernels.

The gather kernel takes only C, ldx, ldo that are multiples of 4: for any other C it runs on a copy padded to the next multiple and the
extra columns are dropped."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import maxpool_refs as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NS, MS, HS, CS = (1, 7, 70, 257), (1, 33, 130), (1, 5, 63, 64, 65, 100, 128, 130), (1, 3, 4, 8, 12, 36, 128)


def G(a, dt=None):
    t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
    return t.to(DEV) if dt is None else t.to(DEV, dt)


def gather_kernel(x, idx, frames=1):
    """cofi_neighbor_maxpool itself (never the router), on a 4-column-padded copy where C is no multiple of 4"""
    from cofii2p_amd import _lib, ops

    lib = _lib.load()
    C = x.shape[1]
    C4 = (C + 3) // 4 * 4
    xp = torch.zeros((x.shape[0], C4), dtype=torch.float32, device=x.device)
    xp[:, :C] = x
    M, H = idx.shape
    out = torch.empty((M, C4), dtype=torch.float32, device=x.device)
    _lib.check(lib.cofi_neighbor_maxpool(ops._p(xp), C4, x.shape[0] // frames, C4, ops._p(idx), M // frames, H, ops._p(out), C4, frames, None,
                                         ops._stream()), "cofi_neighbor_maxpool")
    return out[:, :C]


def same(a, b):
    return torch.equal(a.cpu(), b.cpu() if torch.is_tensor(b) else torch.from_numpy(b))


def check(x, idx, frames=1, order=None, what=""):
    """slice kernel == gather kernel == reference, twice"""
    from cofii2p_amd import ops

    ref = R.neighbor_maxpool_ref(x.cpu().numpy(), idx.cpu().numpy(), frames)
    old = gather_kernel(x, idx, frames)
    for rep in range(2):
        new = ops.neighbor_maxpool_slice(x, idx, frames=frames, order=order)
        assert same(new, old), ("slice vs gather kernel", what, rep)
        assert same(new, ref), ("slice vs reference", what, rep)
    return new


def table(g, N, M, H, frames=1):
    """mostly real neighbours, with shadows (N), duplicates, and indices below 0 and above N"""
    idx = g.integers(0, N, (frames * M, H))
    kind = g.random((frames * M, H))
    idx[kind < 0.15] = N
    idx[(kind >= 0.15) & (kind < 0.20)] = -1 - g.integers(0, 5)
    idx[(kind >= 0.20) & (kind < 0.25)] = N + 1 + g.integers(0, 1000)
    idx[(kind >= 0.25) & (kind < 0.27)] = np.iinfo(np.int32).min + 1   # (the minimum itself is the gather kernel's own mark for "past the row")
    idx[(kind >= 0.27) & (kind < 0.29)] = np.iinfo(np.int32).max
    return idx.astype(np.int32)


@pytest.mark.parametrize("frames", [1, 3])
@pytest.mark.parametrize("H", HS)
def test_every_shape(H, frames):
    """N x M x C at one H and frame count: M above, at and below N; C below one channel group, partial last groups; H around the
    staged chunk (16 / 32 neighbours) and no multiple of 4"""
    g = np.random.default_rng(1000 * H + frames)
    for N in NS:
        for M in MS:
            idx = G(table(g, N, M, H, frames))
            for C in CS:
                x = G(g.standard_normal((frames * N, C)).astype(np.float32))
                check(x, idx, frames, what=(N, M, H, C, frames))


@pytest.mark.parametrize("off", [3, 4])
def test_column_views(off):
    """ldx > C: x a column view of a wider buffer (16-byte aligned or not); out= a column slice of a wider buffer, the rest untouched"""
    from cofii2p_amd import ops

    g = np.random.default_rng(7)
    N, M, H, frames = 70, 33, 65, 3
    for C in (3, 8, 12, 36):
        wide = G(g.standard_normal((frames * N, C + 9)).astype(np.float32))
        x = wide[:, off:off + C]
        idx = G(table(g, N, M, H, frames))
        ref = R.neighbor_maxpool_ref(x.cpu().numpy(), idx.cpu().numpy(), frames)
        old = gather_kernel(x, idx, frames)
        for rep in range(2):
            buf = torch.full((frames * M, C + 11), 7.5, device=DEV)
            got = ops.neighbor_maxpool_slice(x, idx, out=buf[:, off:off + C], frames=frames)
            assert got.data_ptr() == buf[:, off:off + C].data_ptr()
            assert same(buf[:, off:off + C], ref) and same(buf[:, off:off + C], old)
            assert bool((buf[:, :off] == 7.5).all()) and bool((buf[:, off + C:] == 7.5).all())


@pytest.mark.parametrize("H", [1, 5, 64, 130])
def test_zero_row_wins_only_where_a_shadow_is_listed(H):
    """all values negative: a row of shadows gives zeros; one real neighbour + shadows gives zeros; the same real neighbour H times
    (duplicates) gives that row, negative; the shadow in any position of the row"""
    g = np.random.default_rng(H)
    N, C = 70, 12
    x = G(-np.abs(g.standard_normal((N, C))).astype(np.float32) - 0.5)
    rows = [np.full(H, N)]                                   # shadows only
    for pos in {0, H // 2, H - 1}:
        r = np.full(H, 11)
        rows.append(r.copy())                                # duplicates of one real neighbour, no shadow
        if H > 1:
            s = np.full(H, N)
            s[pos] = 11                                      # one real neighbour among shadows
            rows.append(s)
            r[pos] = N                                       # one shadow among real neighbours
            rows.append(r)
    idx = np.stack(rows).astype(np.int32)
    out = check(x, G(idx)).cpu()
    for i, r in enumerate(idx):
        want = torch.zeros(C) if (r == N).any() else x[11].cpu()
        assert torch.equal(out[i], want), (i, r)
    assert bool((out[1] < 0).all())


def test_special_values():
    """+-0, +-inf, the largest and smallest normal and subnormal floats, alone in a row and against each other"""
    fi = np.finfo(np.float32)
    vals = np.array([0.0, -0.0, np.inf, -np.inf, fi.max, -fi.max, fi.tiny, -fi.tiny, fi.smallest_subnormal, -fi.smallest_subnormal,
                     1.0, -1.0], dtype=np.float32)
    N, C = len(vals), 8
    x = np.repeat(vals[:, None], C, 1)
    pairs = np.array([(i, j) for i in range(N) for j in range(N)], dtype=np.int32)          # every value against every value
    single = np.repeat(np.arange(N, dtype=np.int32)[:, None], 2, 1)                         # every value alone (no zero row listed)
    shadow = np.stack([np.arange(N, dtype=np.int32), np.full(N, N, dtype=np.int32)], 1)     # every value against the zero row
    out = check(G(x), G(np.concatenate([pairs, single, shadow]))).cpu().numpy()
    assert np.array_equal(out[len(pairs):len(pairs) + N, 0], vals)                          # alone: the value itself (-0 == 0 numerically)
    assert np.isneginf(out[len(pairs) + 3, 0]) and out[len(pairs) + N + 3, 0] == 0.0        # -inf alone stays; against the zero row: 0


def test_nan_entries_are_skipped_as_in_the_gather_kernel():
    from cofii2p_amd import ops

    g = np.random.default_rng(5)
    N, M, H, C = 70, 33, 65, 12
    x = g.standard_normal((N, C)).astype(np.float32)
    x[g.random((N, C)) < 0.2] = np.nan
    x[5] = np.nan
    idx = table(g, N, M, H)
    idx[0] = 5                                               # a row whose entries are all NaN
    x, idx = G(x), G(idx)
    old = gather_kernel(x, idx)
    for rep in range(2):
        new = ops.neighbor_maxpool_slice(x, idx)
        assert bool(((new == old) | (new.isnan() & old.isnan())).all())
        assert torch.allclose(new, old, rtol=0, atol=0, equal_nan=True)


def test_order_is_ignored():
    g = np.random.default_rng(9)
    N, M, H, C, frames = 257, 130, 100, 36, 3
    x, idx = G(g.standard_normal((frames * N, C)).astype(np.float32)), G(table(g, N, M, H, frames))
    order = G(np.concatenate([g.permutation(M) for _ in range(frames)]).astype(np.int32))
    a = check(x, idx, frames)
    b = check(x, idx, frames, order=order)
    assert torch.equal(a, b)


@pytest.mark.parametrize("frames", [1, 3])
@pytest.mark.parametrize("H", [128, 130])
@pytest.mark.parametrize("C", [4, 12])
@pytest.mark.parametrize("M", [2100, 1029])
def test_query_ranges(M, C, H, frames):
    """few frames, many queries: the entry point splits a frame's queries over S > 1 workgroups per channel group (S = the passes a
    frame needs: 3 and 2 at C = 4 - 64 queries per wave pass -, 5 and 3 at C = 12 - 32 per wave pass), ranges of 700 / 515 / 420 / 343
    queries that are no multiple of a wave pass: range bounds inside a pass, chunks that are full against the frame but not
    against the range"""
    g = np.random.default_rng(M + C + H + frames)
    N = 257
    x, idx = G(g.standard_normal((frames * N, C)).astype(np.float32)), G(table(g, N, M, H, frames))
    check(x, idx, frames, what=(M, C, H, frames))


@pytest.mark.parametrize("C,frames,M,H", [(12, 129, 1100, 5), (12, 129, 1100, 48), (12, 129, 1100, 130), (4, 257, 2100, 5), (4, 257, 2100, 48),
                                          (36, 65, 1025, 5), (36, 65, 1025, 128), (36, 65, 1025, 130)])
def test_several_passes_per_wave(C, frames, M, H):
    """frames x channel groups above 256: one workgroup per (frame, group) walks all M queries, a wave three passes (queries w, w + 512,
    w + 1024 at 8 channels per group; w, w + 1024, w + 2048 at 4): the accumulator starts again after every store, the index loads
    of the next pass's first chunk are issued from the last chunk of this one, the last pass is partial for some waves and past the
    end for the others.  The reference on three of the frames (the first, one inside, the last), the gather kernel on all."""
    from cofii2p_amd import ops

    g = np.random.default_rng(C + frames + H)
    N = 70
    x, idx = G(g.standard_normal((frames * N, C)).astype(np.float32)), G(table(g, N, M, H, frames))
    old = gather_kernel(x, idx, frames)
    for rep in range(2):
        new = ops.neighbor_maxpool_slice(x, idx, frames=frames)
        assert same(new, old), ("slice vs gather kernel", rep)
        for f in (0, frames // 2, frames - 1):
            ref = R.neighbor_maxpool_ref(x[f * N:(f + 1) * N].cpu().numpy(), idx[f * M:(f + 1) * M].cpu().numpy())
            assert same(new[f * M:(f + 1) * M], ref), ("slice vs reference", f, rep)


def _largest_rows(C):
    from cofii2p_amd import ops

    lo, hi = 1, 1 << 20            # ok(lo), not ok(hi)
    assert ops.neighbor_maxpool_slice_ok(lo, C, 5, 1) and not ops.neighbor_maxpool_slice_ok(hi, C, 5, 1)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if ops.neighbor_maxpool_slice_ok(mid, C, 5, 1) else (lo, mid)
    return lo


def test_largest_slice_and_refusal_beyond(monkeypatch):
    """the largest N the query accepts runs and matches (the last source row, the zero row and the -inf row - H = 5 - sit at the very
    end of the slice); N + 1 is refused by the entry point and ops.neighbor_maxpool serves it with the gather kernel"""
    from cofii2p_amd import _lib, ops

    lib = _lib.load()
    g = np.random.default_rng(11)
    M, H, C = 33, 5, 4
    N = _largest_rows(C)
    assert N >= 5120                                         # encoder4_1's source fits
    assert _largest_rows(36) >= 2560                         # encoder5_1's at 8 channels per group (at least)
    for C in (4, 12):
        idx = table(g, N, M, H)
        idx[0] = [N - 1, N - 1, N, N - 2, 0]
        idx[1] = N - 1
        x = G(g.standard_normal((N, C)).astype(np.float32) - 3.0)
        check(x, G(idx), what=("largest", N, C))
    # beyond
    frames = ops.MAXPOOL_SLICE_MIN_FRAMES
    monkeypatch.setattr(ops, "MAXPOOL_SLICE_MAX_ROWS", 1 << 30)        # the kernel's own limit decides, not the routing's
    monkeypatch.delenv("COFI_MAXPOOL_SLICE", raising=False)
    x = G(g.standard_normal((frames * (N + 1), 4)).astype(np.float32))
    idx = G(table(g, N + 1, M, H, frames))
    out = torch.full((frames * M, 4), 3.25, device=DEV)
    assert not ops.neighbor_maxpool_slice_ok(N + 1, 4, H, frames)
    rc = lib.cofi_neighbor_maxpool_slice(ops._p(x), 4, N + 1, 4, ops._p(idx), M, H, ops._p(out), 4, frames, None, ops._stream())
    assert rc == _lib.COFI_EUNSUPPORTED == -3
    torch.cuda.synchronize()
    assert bool((out == 3.25).all())                         # nothing was launched
    with pytest.raises(_lib.CofiError, match="COFI_EUNSUPPORTED"):
        ops.neighbor_maxpool_slice(x, idx, frames=frames)
    for rep in range(2):
        got = ops.neighbor_maxpool(x, idx, frames=frames)
        assert same(got, R.neighbor_maxpool_ref(x.cpu().numpy(), idx.cpu().numpy(), frames)) and same(got, gather_kernel(x, idx, frames))


class Spy:
    """counts the calls of the two C entry points that ops.neighbor_maxpool chooses between"""

    def __init__(self, monkeypatch):
        from cofii2p_amd import _lib

        lib = _lib.load()
        self.calls = {"cofi_neighbor_maxpool": 0, "cofi_neighbor_maxpool_slice": 0}
        for name in self.calls:
            monkeypatch.setattr(lib, name, self._wrap(name, getattr(lib, name)))

    def _wrap(self, name, fn):
        def f(*a):
            self.calls[name] += 1
            return fn(*a)
        return f


def _routed_case(frames):
    g = np.random.default_rng(13)
    N, M, H, C = 257, 130, 128, 36
    return G(g.standard_normal((frames * N, C)).astype(np.float32)), G(table(g, N, M, H, frames)), (N, M, H, C)


def test_routing(monkeypatch):
    """stack mode from MAXPOOL_SLICE_MIN_FRAMES frames and up to MAXPOOL_SLICE_MAX_ROWS rows: the slice kernel; fewer frames, more rows
    or COFI_MAXPOOL_SLICE=0: the gather kernel; the same bits everywhere"""
    from cofii2p_amd import ops

    monkeypatch.delenv("COFI_MAXPOOL_SLICE", raising=False)
    F = ops.MAXPOOL_SLICE_MIN_FRAMES
    spy = Spy(monkeypatch)
    x, idx, _ = _routed_case(F)
    ref = R.neighbor_maxpool_ref(x.cpu().numpy(), idx.cpu().numpy(), F)
    for rep in range(2):
        assert same(ops.neighbor_maxpool(x, idx, frames=F), ref)
    assert spy.calls == {"cofi_neighbor_maxpool": 0, "cofi_neighbor_maxpool_slice": 2}
    monkeypatch.setenv("COFI_MAXPOOL_SLICE", "0")
    assert same(ops.neighbor_maxpool(x, idx, frames=F), ref)
    assert spy.calls == {"cofi_neighbor_maxpool": 1, "cofi_neighbor_maxpool_slice": 2}
    monkeypatch.delenv("COFI_MAXPOOL_SLICE")
    monkeypatch.setattr(ops, "MAXPOOL_SLICE_MAX_ROWS", 256)            # one row too many
    assert same(ops.neighbor_maxpool(x, idx, frames=F), ref)
    assert spy.calls == {"cofi_neighbor_maxpool": 2, "cofi_neighbor_maxpool_slice": 2}
    monkeypatch.undo()
    spy = Spy(monkeypatch)
    x1, idx1, _ = _routed_case(F - 1)                                  # one frame too few
    assert same(ops.neighbor_maxpool(x1, idx1, frames=F - 1), R.neighbor_maxpool_ref(x1.cpu().numpy(), idx1.cpu().numpy(), F - 1))
    assert spy.calls == {"cofi_neighbor_maxpool": 1, "cofi_neighbor_maxpool_slice": 0}


CHILD = r"""
import sys
import numpy as np, torch
sys.path[:0] = [%r, %r]
import maxpool_refs as R
from cofii2p_amd import _lib, ops
lib = _lib.load()
calls = []
for name in ("cofi_neighbor_maxpool", "cofi_neighbor_maxpool_slice"):
    setattr(lib, name, (lambda n, f: lambda *a: (calls.append(n), f(*a))[1])(name, getattr(lib, name)))
F = ops.MAXPOOL_SLICE_MIN_FRAMES
g = np.random.default_rng(13)
x = torch.from_numpy(g.standard_normal((F * 70, 36)).astype(np.float32)).cuda()
idx = torch.from_numpy(g.integers(0, 71, (F * 33, 65)).astype(np.int32)).cuda()
out = ops.neighbor_maxpool(x, idx, frames=F)
assert torch.equal(out.cpu(), torch.from_numpy(R.neighbor_maxpool_ref(x.cpu().numpy(), idx.cpu().numpy(), F)))
print("CALLS", ",".join(calls))
"""


def test_environment_switch_in_a_fresh_process():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, COFI_MAXPOOL_SLICE="0")
    out = subprocess.run([sys.executable, "-c", CHILD % (root, os.path.join(root, "tests"))], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "CALLS cofi_neighbor_maxpool\n" in out.stdout, out.stdout


def test_captured_into_a_graph(monkeypatch):
    """the routed call inside a torch.cuda.graph: no allocation, no attribute call, no synchronisation; two replays on changed inputs"""
    from cofii2p_amd import ops

    F = ops.MAXPOOL_SLICE_MIN_FRAMES
    monkeypatch.delenv("COFI_MAXPOOL_SLICE", raising=False)
    spy = Spy(monkeypatch)
    x, idx, (N, M, H, C) = _routed_case(F)
    out = torch.empty((F * M, C), device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # warm-up outside the capture: code objects are loaded
        ops.neighbor_maxpool(x, idx, out=out, frames=F)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.neighbor_maxpool(x, idx, out=out, frames=F)
    g = np.random.default_rng(17)
    for rep in range(2):
        x.copy_(G(g.standard_normal((F * N, C)).astype(np.float32)))
        idx.copy_(G(table(g, N, M, H, F)))
        out.fill_(-7.0)
        graph.replay()
        torch.cuda.synchronize()
        ref = R.neighbor_maxpool_ref(x.cpu().numpy(), idx.cpu().numpy(), F)
        assert same(out, ref) and same(out, gather_kernel(x, idx, F)), rep
    assert spy.calls["cofi_neighbor_maxpool_slice"] == 2   # the warm-up and the capture
