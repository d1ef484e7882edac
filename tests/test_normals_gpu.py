"""cofi_estimate_normals (csrc/normals.hip) and cofii2p_amd/normals.py on the GPU against the float64 reference of tests/normals_refs.py,
always evaluated on the kernel's own neighbour rows (ops.knn(..., return_dist=True)).  Needs a real MI355X.

Gate (tests/test_normals_refs_cpu.py): a point is compared when gap = (l1 - l0) / l2 >= 0.05; on a compared point
|n x n_ref| <= c(k) 2^-24 / gap with c = 8 up to k = 30 and 32 at k = 128; at most 2 % of the points are left out for k >= 8, 35 % for k = 3.
The kernel's own worst |n x n_ref| gap / 2^-24 on plane_cloud(5), both offsets (recorded from the MI355X run of this file):

      k        3       8      16      30     128
    worst    1.69    1.25    1.46    1.90    2.35      (allowed 8, 8, 8, 8, 32; unit norm within 2.33 x 2^-24)

Sign: compared with the reference on every row where the reference has |n . (v - p)| / |v - p| >= 1e-3 (oriented form) or where its two
largest |components| differ by more than 1e-3 (unoriented form), rows below the gap threshold included: the smallest gap on these clouds is
1.6e-4, where the error bound is still under the 1e-3 margin.  A row that disagrees is printed with its gap and margin."""
import functools

import numpy as np
import pytest
import torch

import normals_refs as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KS = (3, 8, 16, 30, 128)


def G(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def cloud(off):
    return R.plane_cloud(5, offset=R.OFFSETS[off])


@functools.lru_cache(maxsize=None)
def rows(off, k):
    """-> (points, idx, dist) on the device: the self search of the cloud, computed once per (offset, k) and left unchanged"""
    from cofii2p_amd import ops

    pts = G(cloud(off))
    idx, dist = ops.knn(pts, pts, k, return_dist=True)
    return pts, idx, dist


@functools.lru_cache(maxsize=None)
def reference(off, k, oriented=True):
    _, idx, _ = rows(off, k)
    return R.ref_normals64(cloud(off), idx.cpu().numpy(), viewpoint=(0.0, 0.0, 0.0) if oriented else None)


def unit_norm_error(n):
    return np.abs(np.linalg.norm(n.astype(np.float64), axis=1) - 1.0).max() / R.U


def assert_sign_agrees(n, n_ref, rows_checked, margin, lam):
    """n . n_ref > 0 on every checked row; the rows that disagree are printed with their gap and margin first"""
    bad = np.flatnonzero(rows_checked & ((n.astype(np.float64) * n_ref).sum(1) <= 0))
    gap = R.gap_of(lam)
    for i in bad:
        print("row %d: sign differs from the reference, gap %.3g, margin %.3g" % (i, gap[i], margin[i]))
    assert rows_checked.mean() > 0.95 and len(bad) == 0


@pytest.mark.parametrize("off", (0, 1))
@pytest.mark.parametrize("k", KS)
def test_accuracy_unit_norm_and_sign(k, off):
    from cofii2p_amd import normals

    pts, idx, dist = rows(off, k)
    n = normals.normals_from_rows(pts, idx, dist).cpu().numpy()
    n_ref, lam, deg = reference(off, k)
    assert not deg.any()
    worst, left = R.gate(n, n_ref, lam, deg)
    print("k = %d offset %s: worst |n x n_ref| gap / 2^-24 = %.2f (allowed %g), left out %.1f %%, unit norm within %.2f x 2^-24"
          % (k, R.OFFSETS[off], worst, R.KERNEL_C[k], 100 * left, unit_norm_error(n)))
    assert worst <= R.KERNEL_C[k]
    assert left <= R.LEFT_OUT_CAP[k]
    assert unit_norm_error(n) <= 4.0
    to_v = -cloud(off).astype(np.float64)
    dist_v = np.linalg.norm(to_v, axis=1)
    margin = np.abs((n_ref * to_v).sum(1)) / dist_v
    assert_sign_agrees(n, n_ref, margin >= 1e-3, margin, lam)
    assert ((n.astype(np.float64) * to_v).sum(1) >= -1e-6 * dist_v).all()      # no row points away from the viewpoint


@pytest.mark.parametrize("k", (8, 30))
def test_unoriented_form(k):
    from cofii2p_amd import normals

    pts, idx, _ = rows(1, k)
    n = normals.normals_from_rows(pts, idx, viewpoint=None).cpu().numpy()
    n_ref, lam, deg = reference(1, k, oriented=False)
    lead = np.take_along_axis(n, np.argmax(np.abs(n), 1)[:, None], 1)[:, 0]
    assert (lead > 0).all()
    a = np.sort(np.abs(n_ref), 1)
    assert_sign_agrees(n, n_ref, a[:, 2] - a[:, 1] > 1e-3, a[:, 2] - a[:, 1], lam)
    worst, _ = R.gate(n, n_ref, lam, deg)
    assert worst <= R.KERNEL_C[k]
    # the oriented output is the same vector up to its sign
    o = normals.normals_from_rows(pts, idx).cpu().numpy()
    assert np.array_equal(np.abs(o), np.abs(n))


@pytest.mark.parametrize("N", (1, 2, 3))
def test_fewer_points_than_slots(N):
    """rows are shadow-padded (index N); one or two points cannot span a plane, three give a valid one"""
    from cofii2p_amd import normals, ops

    pts = G(cloud(1)[:N])
    idx, dist = ops.knn(pts, pts, 8, return_dist=True)
    assert (idx[:, N:] == N).all()
    count = torch.zeros(1, dtype=torch.int32, device=DEV)
    n = normals.normals_from_rows(pts, idx, dist, degenerate_count=count).cpu().numpy()
    n_ref, lam, deg = R.ref_normals64(cloud(1)[:N], idx.cpu().numpy())
    assert int(count.item()) == deg.sum() == (N if N < 3 else 0)
    if N < 3:
        assert np.array_equal(n, np.tile(np.float32((0.0, 0.0, 1.0)), (N, 1)))
    else:
        worst, left = R.gate(n, n_ref, lam, deg)
        assert left == 0.0 and worst <= R.KERNEL_C[8] and unit_norm_error(n) <= 4.0
        assert ((n * n_ref).sum(1) > 0).all()
    full, cnt = normals.estimate_normals(pts, k=8, return_degenerate=True)     # grid search, the same rows
    assert np.array_equal(full.cpu().numpy(), n) and cnt == int(count.item())


@pytest.mark.parametrize("N", (63, 64, 65, 257))
def test_wave_and_workgroup_tails(N):
    """4 queries per wave, 16 per workgroup: sizes around both, with guard rows behind the output"""
    from cofii2p_amd import normals, ops

    host = cloud(1)[:N]
    pts = G(host)
    idx, dist = ops.knn(pts, pts, 8, return_dist=True)
    buf = torch.full((N + 32, 3), 7.5, dtype=torch.float32, device=DEV)
    n = normals.normals_from_rows(pts, idx, dist, out=buf[:N])
    assert n.data_ptr() == buf.data_ptr() and (buf[N:] == 7.5).all()
    n = n.cpu().numpy()
    n_ref, lam, deg = R.ref_normals64(host, idx.cpu().numpy())
    worst, _ = R.gate(n, n_ref, lam, deg)
    assert not deg.any() and worst <= R.KERNEL_C[8] and unit_norm_error(n) <= 4.0
    assert np.array_equal(normals.estimate_normals(pts, k=8).cpu().numpy(), n)


def test_rows_wider_than_k_and_no_distances():
    from cofii2p_amd import _lib, normals

    pts, idx16, dist16 = rows(0, 16)
    _, idx8, dist8 = rows(0, 8)
    assert torch.equal(idx16[:, :8], idx8)
    want = normals.normals_from_rows(pts, idx8, dist8)
    assert torch.equal(normals.normals_from_rows(pts, idx16[:, :8], dist16[:, :8]), want)      # ldi = 16, k = 8: a view
    assert torch.equal(normals.normals_from_rows(pts, idx16, dist16, k=8), want)               # the same through the k argument
    assert torch.equal(normals.normals_from_rows(pts, idx8, None), want)                       # dist = NULL, no radius
    assert torch.equal(normals.normals_from_rows(pts, idx8, None, radius=0.0), want)
    assert torch.equal(normals.normals_from_rows(pts, idx8, None, radius=-1.0), want)
    with pytest.raises(_lib.CofiError):
        normals.normals_from_rows(pts, idx8, None, radius=0.3)
    lib = _lib.load()
    out = torch.empty((idx8.shape[0], 3), dtype=torch.float32, device=DEV)
    args = (pts.data_ptr(), pts.shape[0], idx8.data_ptr(), None, idx8.shape[0], 8, 8)
    assert lib.cofi_estimate_normals(*args, 0.3, None, out.data_ptr(), 3, 1, None, None) == -1   # COFI_EINVAL: a radius without distances
    assert lib.cofi_estimate_normals(*args[:5], 9, 8, 0.0, None, out.data_ptr(), 3, 1, None, None) == -1   # k > ldi


def test_radius():
    """at most k within radius: the radius is the median distance to the 4th neighbour, so that a sizeable share of the rows keeps fewer than
    three slots (the point itself and at most one neighbour)"""
    from cofii2p_amd import normals

    pts, idx, dist = rows(0, 16)
    d = dist.cpu().numpy()
    radius = float(np.sqrt(np.median(d[:, 4])))
    r2 = np.float32(radius) * np.float32(radius)                 # what the entry point compares with
    keep = d <= r2
    n_ref, lam, deg = R.ref_normals64(cloud(0), idx.cpu().numpy(), keep_mask=keep)
    assert 0.05 < deg.mean() < 0.5
    count = torch.zeros(1, dtype=torch.int32, device=DEV)
    n = normals.normals_from_rows(pts, idx, dist, radius=radius, degenerate_count=count).cpu().numpy()
    assert int(count.item()) == deg.sum()
    assert np.array_equal(n[deg], np.tile(np.float32((0.0, 0.0, 1.0)), (int(deg.sum()), 1)))
    assert not (n[~deg] == np.float32((0.0, 0.0, 1.0))).all(1).any()
    # the kept sets are the reference's: every row with a defined normal agrees with the reference on ITS mask (3 .. 16 slots kept)
    gap = R.gap_of(lam)
    cmp_rows = ~deg & (gap >= R.GAP_MIN)
    err = R.cross_err(n[cmp_rows], n_ref[cmp_rows]) * gap[cmp_rows] / R.U
    assert cmp_rows.sum() > 400 and err.max() <= R.KERNEL_C[16]
    assert unit_norm_error(n) <= 4.0
    full, cnt = normals.estimate_normals(pts, k=16, radius=radius, return_degenerate=True)
    assert np.array_equal(full.cpu().numpy(), n) and cnt == deg.sum()


def test_degenerate_geometry():
    from cofii2p_amd import normals

    g = np.random.default_rng(9)
    same = G(np.tile(np.float32((12.5, -3.25, 0.75)), (64, 1)))
    n, cnt = normals.estimate_normals(same, k=8, return_degenerate=True)
    assert cnt == 64 and np.array_equal(n.cpu().numpy(), np.tile(np.float32((0.0, 0.0, 1.0)), (64, 1)))

    axis = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    line = (np.array([3.0, -2.0, 1.0]) + 0.1 * np.arange(64)[:, None] * axis).astype(np.float32)
    n = normals.estimate_normals(G(line), k=8).cpu().numpy().astype(np.float64)
    assert np.isfinite(n).all() and unit_norm_error(n) <= 4.0
    assert np.abs(n @ axis).max() <= 1e-5                         # perpendicular to the line; the direction around it is free

    flat = np.concatenate([g.uniform(-4.0, 4.0, (200, 2)), np.zeros((200, 1))], 1).astype(np.float32)    # z = 0 exactly: l0 = 0
    for k in (8, 30):
        n, cnt = normals.estimate_normals(G(flat), k=k, return_degenerate=True)
        n = n.cpu().numpy().astype(np.float64)
        assert cnt == 0 and np.linalg.norm(np.cross(n, (0.0, 0.0, 1.0)), axis=1).max() <= 1e-6
        assert (np.abs(n[:, 2]) > 0.999999).all()


def test_strided_output_and_reproducibility():
    from cofii2p_amd import normals

    pts, idx, dist = rows(1, 30)
    N = pts.shape[0]
    want = normals.normals_from_rows(pts, idx, dist)
    assert torch.equal(normals.normals_from_rows(pts, idx, dist), want)        # two launches, equal bits
    scan = torch.full((7, N), -3.0, dtype=torch.float32, device=DEV)
    got = normals.normals_from_rows(pts, idx, dist, out=scan[4:7].t())         # rows 4..6 of a channel-major scan, in place
    assert got.data_ptr() == scan[4].data_ptr()
    assert torch.equal(scan[4:7].t().contiguous(), want) and (scan[:4] == -3.0).all()
    scan2 = torch.full((7, N), -3.0, dtype=torch.float32, device=DEV)
    normals.estimate_normals(pts, k=30, out=scan2[4:7].t())
    assert torch.equal(scan2, scan)
    assert torch.equal(normals.estimate_normals(pts, k=30), want)              # grid rows = brute-force rows
    from cofii2p_amd import ops
    assert torch.equal(normals.estimate_normals(pts, k=30, grid=ops.KnnGrid(pts)), want)
    empty = normals.estimate_normals(torch.empty((0, 3), dtype=torch.float32, device=DEV))
    assert tuple(empty.shape) == (0, 3)


def test_errors_are_raised_before_any_launch(monkeypatch):
    from cofii2p_amd import _lib, normals

    pts, _, _ = rows(0, 8)
    wide = torch.zeros((64, 4), dtype=torch.float32, device=DEV)
    _lib.load()

    def no_load():
        raise AssertionError("an invalid call reached the library")

    monkeypatch.setattr(_lib, "load", no_load)
    for bad in (dict(points=pts, k=0), dict(points=pts, k=129), dict(points=wide[:, :3]), dict(points=pts.double()),
                dict(points=pts.cpu()), dict(points=pts, radius=0.0)):
        with pytest.raises(_lib.CofiError):
            normals.estimate_normals(**bad)
