"""References for the surface-normal estimator (csrc/normals.hip, cofii2p_amd/normals.py), shared by tests/test_normals_refs_cpu.py -
which pins the float32 restatement against the float64 reference - and tests/test_normals_gpu.py - which judges the HIP kernel by the
same float64 reference.  Plain numpy on the CPU throughout.

    plane_cloud     the three-plane test cloud (floor + two walls, sigma of noise across each plane)
    brute_knn       exact brute-force neighbours in float64, ascending (distance, index), shadow-padded like the device search
    ref_normals64   float64: mean-centred covariance + numpy.linalg.eigh, the kernel's degenerate and orientation rules
    restate32       float32: query-centred one-pass covariance + float32 eigh (what a careful fp32 implementation can reach)
    cross_err       |n x n_ref| with n renormalised in float64 (sqrt(1 - dot^2) has a floor near 3e-4 for float32 unit vectors)
    bound           the accuracy gate c(k) 2^-24 / gap, gap = (l1 - l0) / l2
"""
import numpy as np

U = 2.0 ** -24          # unit roundoff of float32
GAP_MIN = 0.05          # a point is compared only when (l1 - l0) / l2 >= GAP_MIN
# worst |n x n_ref| gap / 2^-24 of restate32 on plane_cloud(5), offsets (0,0,0) and (60,-40,0), exact neighbours (measured on the CPU)
RESTATE_WORST = {3: 1.57, 8: 1.28, 16: 1.75, 30: 1.96, 128: 7.23}
# the kernel's allowance: 4 x the restatement's worst figure, i.e. 8 up to k = 30 and 32 at k = 128
KERNEL_C = {3: 8.0, 8: 8.0, 16: 8.0, 30: 8.0, 128: 32.0}
LEFT_OUT_CAP = {3: 0.35, 8: 0.02, 16: 0.02, 30: 0.02, 128: 0.02}
OFFSETS = ((0.0, 0.0, 0.0), (60.0, -40.0, 0.0))


def plane_cloud(seed, n=1536, offset=(0.0, 0.0, 0.0), sigma=0.02):
    """n // 2 points on the floor z = -1.73, n // 4 on the wall x = 6, the rest on the wall y = 6 (each with N(0, sigma) across the
    plane), permuted, shifted by `offset`, float32 (n, 3)."""
    g = np.random.default_rng(seed)
    nf, nw = n // 2, n // 4
    nv = n - nf - nw
    floor = np.stack([g.uniform(0.0, 6.0, nf), g.uniform(0.0, 6.0, nf), -1.73 + g.normal(0.0, sigma, nf)], 1)
    wall_x = np.stack([6.0 + g.normal(0.0, sigma, nw), g.uniform(0.0, 6.0, nw), g.uniform(-1.73, 2.27, nw)], 1)
    wall_y = np.stack([g.uniform(0.0, 6.0, nv), 6.0 + g.normal(0.0, sigma, nv), g.uniform(-1.73, 2.27, nv)], 1)
    pts = np.concatenate([floor, wall_x, wall_y], 0)[g.permutation(n)]
    return np.ascontiguousarray((pts + np.asarray(offset, dtype=np.float64)).astype(np.float32))


def brute_knn(points, k):
    """-> idx (N, k) int64, d2 (N, k) float64: the k nearest rows of `points` per row (itself included), ascending (distance, index);
    slots past the cloud hold the shadow index N and +inf."""
    p = np.asarray(points, dtype=np.float64)
    n = p.shape[0]
    d2 = ((p[:, None, :] - p[None, :, :]) ** 2).sum(2)
    order = np.lexsort((np.broadcast_to(np.arange(n), (n, n)), d2), axis=1)[:, :k]
    idx = np.full((n, k), n, dtype=np.int64)
    dist = np.full((n, k), np.inf)
    idx[:, :order.shape[1]] = order
    dist[:, :order.shape[1]] = np.take_along_axis(d2, order, 1)
    return idx, dist


def canonical_sign(n):
    """the component of largest magnitude positive, lowest axis on ties"""
    a = np.abs(n)
    pick = np.argmax(a, axis=1)                    # argmax returns the first maximum: lowest axis on ties
    s = np.take_along_axis(n, pick[:, None], 1)[:, 0]
    return np.where(s < 0, -1.0, 1.0)[:, None] * n


def orient(n, points, viewpoint):
    """the kernel's sign rule: canonical sign, then (with a viewpoint v) flipped when n . (v - p) < 0"""
    n = canonical_sign(n)
    if viewpoint is None:
        return n
    to_v = np.asarray(viewpoint, dtype=np.float64)[None, :] - np.asarray(points, dtype=np.float64)
    return np.where(((n * to_v).sum(1) < 0)[:, None], -n, n)


def ref_normals64(points, idx, keep_mask=None, viewpoint=(0.0, 0.0, 0.0)):
    """float64 reference on the neighbour rows `idx` (Q, k) into points (S, 3); row q belongs to point q.  A slot counts when its index is
    < S and keep_mask (Q, k), if given, is true.  -> (normals (Q, 3), eigenvalues (Q, 3) ascending, degenerate (Q,) bool); a row is degenerate
    with fewer than 3 slots, trace(C) == 0 or a non-finite result, and then holds (0, 0, 1) and zero eigenvalues."""
    p = np.asarray(points, dtype=np.float64)
    idx = np.asarray(idx).astype(np.int64)
    S, (Q, k) = p.shape[0], idx.shape
    keep = (idx >= 0) & (idx < S)
    if keep_mask is not None:
        keep &= np.asarray(keep_mask, dtype=bool)
    w = keep[:, :, None].astype(np.float64)
    d = (p[np.clip(idx, 0, S - 1)] - p[:Q, None, :]) * w           # query-centred first: exact for float32 inputs that are close
    m = keep.sum(1)
    mm = np.maximum(m, 1)[:, None]
    d = (d - d.sum(1, keepdims=True) / mm[:, :, None]) * w
    C = np.einsum("qki,qkj->qij", d, d) / mm[:, :, None]
    tr = np.trace(C, axis1=1, axis2=2)
    deg = (m < 3) | (tr == 0) | ~np.isfinite(tr)
    C[deg] = np.identity(3)
    lam, vec = np.linalg.eigh(C)
    n = vec[:, :, 0]
    deg |= ~np.isfinite(n).all(1)
    n = orient(np.where(deg[:, None], 0.0, n), p[:Q], viewpoint)
    n[deg] = (0.0, 0.0, 1.0)
    lam[deg] = 0.0
    return n, lam, deg


def restate32(points, idx):
    """float32 restatement, every slot valid: d = neighbour - query, one pass over the slots accumulating sum d and sum d d^T in float32,
    C = sum d d^T / k - (sum d / k)(sum d / k)^T, float32 eigh.  -> unit eigenvector of the smallest eigenvalue (Q, 3), sign free."""
    p = np.asarray(points, dtype=np.float32)
    idx = np.asarray(idx).astype(np.int64)
    Q, k = idx.shape
    s = np.zeros((Q, 3), dtype=np.float32)
    ss = np.zeros((Q, 3, 3), dtype=np.float32)
    for j in range(k):
        d = p[idx[:, j]] - p[:Q]
        s += d
        ss += d[:, :, None] * d[:, None, :]
    kf = np.float32(k)
    mean = s / kf
    C = ss / kf - mean[:, :, None] * mean[:, None, :]
    assert C.dtype == np.float32
    _, vec = np.linalg.eigh(C)
    assert vec.dtype == np.float32
    return vec[:, :, 0]


def cross_err(n, n_ref):
    """|n x n_ref| per row, n renormalised in float64"""
    a = np.asarray(n, dtype=np.float64)
    a = a / np.linalg.norm(a, axis=1, keepdims=True)
    return np.linalg.norm(np.cross(a, np.asarray(n_ref, dtype=np.float64)), axis=1)


def gap_of(lam):
    """(l1 - l0) / l2 of ascending eigenvalues (0 where l2 == 0)"""
    return np.where(lam[:, 2] > 0, (lam[:, 1] - lam[:, 0]) / np.where(lam[:, 2] > 0, lam[:, 2], 1.0), 0.0)


def gate(n, n_ref, lam, deg=None):
    """-> (worst |n x n_ref| gap / 2^-24 over the compared rows, share of rows left out): a row is compared when it is not degenerate and
    gap >= GAP_MIN"""
    gap = gap_of(lam)
    cmp_rows = gap >= GAP_MIN
    if deg is not None:
        cmp_rows &= ~deg
    err = cross_err(n, n_ref)
    worst = float((err[cmp_rows] * gap[cmp_rows] / U).max()) if cmp_rows.any() else 0.0
    return worst, 1.0 - float(cmp_rows.mean())
