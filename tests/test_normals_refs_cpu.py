"""The references the normal estimator is judged by (tests/normals_refs.py), on the CPU: the float32 restatement against the float64
reference on the three-plane cloud, which fixes the accuracy gate of tests/test_normals_gpu.py.

A point is compared when gap = (l1 - l0) / l2 >= 0.05 (float64 eigenvalues); the bound on a compared point is |n x n_ref| <= c(k) 2^-24 / gap,
the eigenvector perturbation bound for an fp32-rounded covariance.  Figures on plane_cloud(5), offsets (0,0,0) and (60,-40,0), exact
brute-force neighbours, worst |n x n_ref| gap / 2^-24 of restate32 and share of points left out:

      k      worst   left out
      3      1.57    30.4 %     (three points always span a plane; a near-collinear triple has no defined normal: cap 35 %)
      8      1.28     0.8 %     (cap for k >= 8: 2 %)
     16      1.75     0
     30      1.96     0
    128      7.23     0

The kernel is allowed c(k) = 4 x the restatement's worst figure: 8 up to k = 30, 32 at k = 128 (normals_refs.KERNEL_C)."""
import functools

import numpy as np
import pytest
import torch

import normals_refs as R

KS = (3, 8, 16, 30, 128)


@functools.lru_cache(maxsize=None)
def measured(k):
    """-> [(worst figure, left-out share)] of restate32 per offset"""
    res = []
    for off in R.OFFSETS:
        pts = R.plane_cloud(5, offset=off)
        idx, _ = R.brute_knn(pts, k)
        n_ref, lam, deg = R.ref_normals64(pts, idx)
        assert not deg.any()
        res.append(R.gate(R.restate32(pts, idx), n_ref, lam, deg))
    return res


@pytest.mark.parametrize("k", KS)
def test_restatement_figures_are_the_recorded_ones(k):
    res = measured(k)
    worst = max(w for w, _ in res)
    print("k = %d: worst |n x n_ref| gap / 2^-24 = %.2f, left out %s" % (k, worst, ["%.1f %%" % (100 * s) for _, s in res]))
    assert R.RESTATE_WORST[k] / 1.5 <= worst <= R.RESTATE_WORST[k] * 1.5
    for _, left in res:
        assert left <= R.LEFT_OUT_CAP[k]
    assert R.KERNEL_C[k] == (32.0 if k == 128 else 8.0) and R.KERNEL_C[k] >= 4.0 * R.RESTATE_WORST[k]


def test_left_out_shares_are_the_recorded_ones():
    assert abs(max(s for _, s in measured(3)) - 0.304) < 0.02
    assert abs(max(s for _, s in measured(8)) - 0.008) < 0.004
    for k in (16, 30, 128):
        assert max(s for _, s in measured(k)) == 0.0


def test_plane_cloud_is_the_stated_generator():
    pts = R.plane_cloud(5)
    assert pts.dtype == np.float32 and pts.shape == (1536, 3) and np.array_equal(pts, R.plane_cloud(5))
    floor = np.abs(pts[:, 2] + 1.73) < 0.15
    wall_x = np.abs(pts[:, 0] - 6.0) < 0.15
    wall_y = np.abs(pts[:, 1] - 6.0) < 0.15
    # 768 / 384 / 384 points, plus the few of another plane that lie within 0.15 m of the edge where two planes meet
    assert 768 <= floor.sum() <= 828 and 384 <= wall_x.sum() <= 444 and 384 <= wall_y.sum() <= 444
    shifted = R.plane_cloud(5, offset=(60.0, -40.0, 0.0))
    assert np.abs(shifted.astype(np.float64) - (pts.astype(np.float64) + np.array([60.0, -40.0, 0.0]))).max() < 1e-5


def test_reference_rules():
    """degenerate rows, the radius mask, the shadow index and the two sign rules of the float64 reference"""
    g = np.random.default_rng(0)
    flat = np.concatenate([g.uniform(-1.0, 1.0, (40, 2)), np.full((40, 1), 2.0)], 1).astype(np.float32)   # the plane z = 2 above the origin
    idx, d2 = R.brute_knn(flat, 8)
    n, lam, deg = R.ref_normals64(flat, idx)
    assert not deg.any() and np.allclose(n, (0.0, 0.0, -1.0)) and np.allclose(lam[:, 0], 0.0)        # towards the viewpoint at the origin
    n, _, _ = R.ref_normals64(flat, idx, viewpoint=None)
    assert np.allclose(n, (0.0, 0.0, 1.0))                                                           # largest component positive
    n, _, deg = R.ref_normals64(flat, idx, keep_mask=d2 <= 0.0)                                      # only the point itself is kept
    assert deg.all() and np.array_equal(n, np.tile((0.0, 0.0, 1.0), (40, 1)))
    two = flat[:2]
    idx, d2 = R.brute_knn(two, 8)
    assert (idx[:, 2:] == 2).all() and np.isinf(d2[:, 2:]).all()
    assert R.ref_normals64(two, idx)[2].all()
    same = np.tile(flat[:1], (8, 1))
    assert R.ref_normals64(same, R.brute_knn(same, 8)[0])[2].all()
    tie = R.canonical_sign(np.array([[-0.5, 0.5, 0.0], [0.5, -0.5, 0.0], [0.0, -0.6, 0.6]]))
    assert np.array_equal(tie, [[0.5, -0.5, 0.0], [0.5, -0.5, 0.0], [0.0, 0.6, -0.6]])                # lowest axis on ties
    a = np.array([[0.0, 0.0, 1.0]])
    assert R.cross_err(2.0 * a, a)[0] == 0.0 and abs(R.cross_err(np.array([[1e-6, 0.0, 1.0]]), a)[0] - 1e-6) < 1e-12


def test_entry_point_is_declared_and_bound():
    from cofii2p_amd import _lib

    assert "cofi_estimate_normals" in _lib.SIGNATURES
    assert "cofi_estimate_normals" in _lib.header_symbols()
    assert len(_lib.SIGNATURES["cofi_estimate_normals"][1]) == 14


def test_python_interface_rejects_host_tensors_before_loading_anything(monkeypatch):
    from cofii2p_amd import _lib, normals

    def no_load():
        raise AssertionError("the library was loaded for an invalid call")

    monkeypatch.setattr(_lib, "load", no_load)
    with pytest.raises(_lib.CofiError):
        normals.estimate_normals(torch.zeros((8, 3)))
    with pytest.raises(_lib.CofiError):
        normals.estimate_normals(np.zeros((8, 3), dtype=np.float32))
