"""The stop rule of the SORTED KPConv aggregation kernels (csrc/kpconv.hip, kp_prefix_done) on the CPU: numpy-float32 emulations
(tests/kpconv_prefix_ref.py) of the canonical KNN distance the rows are sorted by, of the kernels' support test and of the rule.  On rows
sorted by the emulated canonical distance the chunked gather must read every neighbour the unsorted kernels keep - ZERO rows may stop
before their last survivor; this is a condition, not a tolerance.  And the flag bit table against row_pos.  No GPU, no built library."""
import numpy as np
import pytest

import kpconv_prefix_ref as R

F = np.float32
HS = (4, 12, 16, 20, 64, 100, 128)
QNORMS = (0.0, 1e-3, 1.0, 30.0, 100.0, 1e3, 1e4)
RSUPS = (0.48, 0.96, 1.92, 3.84, 7.69)   # the support radii of the encoder's five stages
COUNTS = (0, 1, 15, 16, 17, 63, 64, 65, 128)


def _rsup2(rsup):
    """the kernel's squared support radius for a kernel-point table of largest norm 0.6 rsup and sigma = 0.4 rsup"""
    kp = np.zeros((15, 3), dtype=F)
    kp[1:, 0] = np.linspace(0.1, 0.6, 14) * rsup
    return R.support_radius2(kp, 0.4 * rsup)


def _dirs(g, shape):
    d = g.standard_normal(shape + (3,))
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


def _queries(g, rows, qnorm):
    return (_dirs(g, (rows,)) * qnorm).astype(F)


def _check(q, s, nvalid, rsup2, want_counts=None):
    """sorts the rows, runs the emulated gather -> the rows' survivor counts; asserts that no row stops before its last survivor"""
    rows, H = s.shape[:2]
    # shadow entries: behind the valid ones, whatever lies at their positions must not matter - give them the query's own position
    idx = np.broadcast_to(np.arange(H), (rows, H)).copy()
    tail = idx >= nvalid[:, None]
    s_sorted, idx_sorted = R.sort_rows(q, np.where(tail[..., None], np.float32(1e18), s), idx)   # 1e18: behind every valid entry
    valid_sorted = np.arange(H)[None, :] < nvalid[:, None]
    assert ((idx_sorted < nvalid[:, None]) == valid_sorted).all()   # the valid entries came first
    s_sorted = np.where(valid_sorted[..., None], s_sorted, q[:, None, :])   # what a shadow's row-0 gather may return: anything
    keep = R.survivors(q, s_sorted, nvalid, rsup2)
    nin = keep.sum(1)
    last = np.where(nin > 0, H - np.argmax(keep[:, ::-1], axis=1), 0)   # one past the last survivor
    got = R.gathered(q, s_sorted, nvalid, rsup2)
    early = int((got < last).sum())
    assert early == 0, "%d of %d rows stop before their last survivor" % (early, rows)
    # (the survivors need not be the first nin entries: far from the origin the canonical distance orders near neighbours by its own
    # rounding - the rule then reads on, and the compaction keeps the row's order among what was read)
    assert ((got == H) | np.isin(got, R.CHUNK_ENDS)).all()
    if want_counts is not None:
        assert (nin == want_counts).all()
    return nin, got


@pytest.mark.parametrize("H", HS)
def test_random_rows_every_shadow_tail(H):
    """distances uniform in [0, 3 rsup]; every number of valid entries 0 .. H; |q| from 0 to 1e4 m.  At least 30 000 rows per H: more
    than 200 000 over the seven H"""
    g = np.random.default_rng(H)
    total = 0
    for qnorm in QNORMS:
        for rsup in RSUPS:
            reps = -(-860 // (H + 1))
            nvalid = np.tile(np.arange(H + 1), reps)
            rows = len(nvalid)
            total += rows
            q = _queries(g, rows, qnorm)
            s = (q[:, None, :].astype(np.float64) + _dirs(g, (rows, H)) * g.uniform(0, 3 * rsup, (rows, H, 1))).astype(F)
            _check(q, s, nvalid, _rsup2(rsup))
    assert total >= 30000


@pytest.mark.parametrize("H", HS)
def test_chosen_survivor_counts(H):
    """rows with exactly 0, 1, 15, 16, 17, 63, 64, 65 and 128 survivors (as far as H allows), the others just outside and further out"""
    g = np.random.default_rng(100 + H)
    for qnorm in (0.0, 1.0, 100.0):   # further out the fp32 grid of the coordinates is coarser than the 1 % gap below
        for rsup in RSUPS:
            rsup2 = _rsup2(rsup)
            rk = float(np.sqrt(rsup2))
            for n in [c for c in COUNTS if c <= H]:
                rows = 24
                q = _queries(g, rows, qnorm)
                dist = np.concatenate([g.uniform(0.0, 0.99, (rows, n)), g.uniform(1.01, 3.0, (rows, H - n))], 1) * rk
                dist[:, n:n + 2] = 1.01 * rk   # the first ones outside hug the support
                s = (q[:, None, :].astype(np.float64) + _dirs(g, (rows, H)) * dist[..., None]).astype(F)
                nvalid = np.full(rows, H)
                nvalid[::4] = g.integers(n, H + 1, len(nvalid[::4]))   # some rows with a shadow tail behind the survivors
                nin, got = _check(q, s, nvalid, rsup2, want_counts=n)
                if n <= 15 and qnorm <= 1.0 and H >= 16:
                    assert (got[nvalid == H] == 16).all()   # near the origin a 1 % gap is enough to stop after the first chunk


@pytest.mark.parametrize("H", HS)
def test_boundary_huggers(H):
    """neighbours within 1e-6 relative of the support radius on both sides, around queries at every distance from the origin"""
    g = np.random.default_rng(200 + H)
    for qnorm in QNORMS:
        for rsup in RSUPS:
            rsup2 = _rsup2(rsup)
            rk = float(np.sqrt(rsup2))
            rows = 48
            q = _queries(g, rows, qnorm)
            rel = g.uniform(-1e-6, 1e-6, (rows, H))
            rel[:, ::5] = g.choice([-1e-6, -1e-7, 0.0, 1e-7, 1e-6], (rows, len(range(0, H, 5))))
            far = g.random((rows, H)) < 0.25
            dist = np.where(far, g.uniform(0, 3, (rows, H)), 1.0 + rel) * rk
            s = (q[:, None, :].astype(np.float64) + _dirs(g, (rows, H)) * dist[..., None]).astype(F)
            nvalid = g.integers(0, H + 1, rows)
            nvalid[::3] = H
            _check(q, s, nvalid, rsup2)


@pytest.mark.parametrize("H", HS)
def test_ties_and_duplicates(H):
    """sub-sampling draws with replacement: neighbour rows that repeat a few points, the query among them, and points mirrored to the
    same distance"""
    g = np.random.default_rng(300 + H)
    for qnorm in QNORMS:
        for rsup in RSUPS:
            rows, pool = 48, max(3, H // 6)
            q = _queries(g, rows, qnorm)
            base = (q[:, None, :].astype(np.float64) + _dirs(g, (rows, pool)) * g.uniform(0, 2 * rsup, (rows, pool, 1))).astype(F)
            base[:, 0] = q                                   # the query itself: distance 0, clamped by the canonical form
            base[:, 1] = (2 * q.astype(np.float64) - base[:, 2].astype(np.float64)).astype(F)   # mirror image of point 2
            pick = g.integers(0, pool, (rows, H))
            s = np.take_along_axis(base, pick[..., None], 1)
            nvalid = g.integers(0, H + 1, rows)
            nvalid[::2] = H
            _check(q, s, nvalid, _rsup2(rsup))


def test_dense_cluster_and_far_field():
    """all 128 inside (every chunk is read), and rows whose nearest neighbour is already outside (one chunk, nothing kept)"""
    g = np.random.default_rng(7)
    for qnorm in QNORMS:
        for rsup in RSUPS:
            rsup2 = _rsup2(rsup)
            rk = float(np.sqrt(rsup2))
            rows, H = 32, 128
            q = _queries(g, rows, qnorm)
            grid = max(float(np.spacing(F(qnorm))), 0.0)   # coordinates near q move in steps of this size
            if 0.9 * rk > 8 * grid:
                s = (q[:, None, :].astype(np.float64) + _dirs(g, (rows, H)) * g.uniform(0, 0.9 * rk - 4 * grid, (rows, H, 1))).astype(F)
                nin, got = _check(q, s, np.full(rows, H), rsup2, want_counts=H)
                assert (got == H).all()
            s = (q[:, None, :].astype(np.float64) + _dirs(g, (rows, H)) * g.uniform(1.5 * rk + 4 * grid, 4 * rk + 8 * grid, (rows, H, 1))).astype(F)
            nin, got = _check(q, s, np.full(rows, H), rsup2, want_counts=0)
            if qnorm <= 100.0:
                assert (got == 16).all()


def test_rule_needs_more_than_the_radius():
    """the rule never lets a wave stop behind a neighbour that is itself inside the support, and gives up (reads on) far from the origin
    where the fp32 distances no longer order the row reliably"""
    rsup2 = _rsup2(0.48)
    q = np.zeros((4, 3), dtype=F)
    d2 = np.array([0.0, 0.5 * rsup2, rsup2, np.nextafter(F(rsup2), F(np.inf))], dtype=F)
    assert not R.prefix_done(d2, q, rsup2).any()
    assert R.prefix_done(np.array([1.01 * rsup2], dtype=F), q[:1], rsup2).all()
    far = np.array([[1e4, 0, 0]], dtype=F)
    assert not R.prefix_done(np.array([4 * rsup2], dtype=F), far, rsup2).any()


@pytest.mark.parametrize("N", [1, 31, 32, 33, 63, 64, 65, 100])
@pytest.mark.parametrize("frames", [1, 3])
def test_bit_table_equals_row_pos(N, frames):
    g = np.random.default_rng(N + 1000 * frames)
    for fill in ("mixed", "zeros", "ones"):
        rp = {"mixed": g.integers(0, 2, (frames, N)), "zeros": np.zeros((frames, N), dtype=np.int64), "ones": np.ones((frames, N), dtype=np.int64)}[fill]
        bits = R.pack_bits(rp)
        assert bits.shape == (frames, (N + 31) // 32) and bits.dtype == np.uint32
        n = np.arange(N)
        assert (((bits[:, n >> 5] >> (n & 31).astype(np.uint32)) & 1) == rp).all()     # per frame: frame f's word n >> 5
        pad = np.arange(N, bits.shape[1] * 32)
        assert (((bits[:, pad >> 5] >> (pad & 31).astype(np.uint32)) & 1) == 0).all()   # padding bits
        assert (R.pack_bits_as_launched(rp) == bits).all()
