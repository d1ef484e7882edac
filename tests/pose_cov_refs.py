"""Float64 numpy restatement (TEST INFRASTRUCTURE ONLY) of the pose covariance ("Pose uncertainty"; csrc/pnp.hip,
cofi_pose_covariance*, cofi_pose_nees), built on oracle/pnp_oracle.py and tests/rig_pose_refs.py, plus the scenes the CPU and the GPU
tests share.

Conventions are those of tests/rig_pose_refs.py: a pose is (R (3,3), t (3,)) or 12 numbers R row-major | t, cloud -> camera; E (3,4) =
[R_c | t_c], camera <- rig; the tangent vector is (omega, v) of R' = exp(omega) R, t' = exp(omega) t + v.  A body is a list of cameras,
each a dict(X (n,3), uv (n,2), K4, mask (n,), E (3,4) or None); None is the frame form.

Per row the residual and the 2 x 6 Jacobian are written operation by operation as csrc/pnp.hip::accumulate / accumulate_rig write them
(IEEE fp64, no contraction on either side), so a row contributes the same bits here and on the device; what differs is the order of the
sums, which is what the tolerances below account for."""
import numpy as np

import pnp_oracle as po
import rig_pose_refs as rr

U = 2.0 ** -52
PIVOT_MIN = 1e-12


# ------------------------------------------------------------------------------------------------ the definition
def row_terms(R, t, X, uv, K4, E=None):
    """-> (r (n,2), J (n,2,6), depth (n,)) of every row under the pose (R, t): of the camera itself (E None), or of the RIG with the row
    seen through E"""
    fx, fy, cx, cy = (np.float64(np.float32(k)) for k in K4)
    X, uv = np.asarray(X, np.float64).reshape(-1, 3), np.asarray(uv, np.float64).reshape(-1, 2)
    X0, X1, X2 = X[:, 0], X[:, 1], X[:, 2]
    xr = R[0, 0] * X0 + R[0, 1] * X1 + R[0, 2] * X2 + t[0]
    yr = R[1, 0] * X0 + R[1, 1] * X1 + R[1, 2] * X2 + t[1]
    zr = R[2, 0] * X0 + R[2, 1] * X1 + R[2, 2] * X2 + t[2]
    if E is None:
        x, y, z = xr, yr, zr
    else:
        e = np.concatenate([np.asarray(E, np.float64)[:, :3].reshape(9), np.asarray(E, np.float64)[:, 3]])
        x = e[0] * xr + e[1] * yr + e[2] * zr + e[9]
        y = e[3] * xr + e[4] * yr + e[5] * zr + e[10]
        z = e[6] * xr + e[7] * yr + e[8] * zr + e[11]
    with np.errstate(all="ignore"):
        iz = 1.0 / z
        r = np.stack([fx * x * iz + cx - uv[:, 0], fy * y * iz + cy - uv[:, 1]], 1)
        a00, a02, a11, a12 = fx * iz, -fx * x * iz * iz, fy * iz, -fy * y * iz * iz
        zero = np.zeros_like(z)
        if E is None:
            J0 = [a02 * y, a00 * z - a02 * x, -a00 * y, a00, zero, a02]
            J1 = [-a11 * z + a12 * y, -a12 * x, a11 * x, zero, a11, a12]
        else:
            A0 = [a00 * e[j] + a02 * e[6 + j] for j in range(3)]
            A1 = [a11 * e[3 + j] + a12 * e[6 + j] for j in range(3)]
            J0 = [A0[2] * yr - A0[1] * zr, A0[0] * zr - A0[2] * xr, A0[1] * xr - A0[0] * yr, A0[0], A0[1], A0[2]]
            J1 = [A1[2] * yr - A1[1] * zr, A1[0] * zr - A1[2] * xr, A1[1] * xr - A1[0] * yr, A1[0], A1[1], A1[2]]
    J = np.stack([np.stack(J0, 1), np.stack(J1, 1)], 1)
    return r, J, z


def normal_equations(pose12, cams):
    """the rows used and their sums -> dict(H, cost, n, absH = sum |J_ki| |J_kj|, any_camera)"""
    p = np.asarray(pose12, np.float64).reshape(12)
    R, t = p[:9].reshape(3, 3), p[9:]
    H, absH, cost, n, any_camera = np.zeros((6, 6)), np.zeros((6, 6)), 0.0, 0, False
    for cam in cams:
        if not rr.usable(cam["K4"]):
            continue
        any_camera = True
        if len(cam["X"]) == 0:
            continue
        r, J, z = row_terms(R, t, cam["X"], cam["uv"], cam["K4"], cam.get("E"))
        with np.errstate(invalid="ignore"):
            use = (np.asarray(cam["mask"]) != 0) & (z > 1e-6)
        Jf, rf = J[use].reshape(-1, 6), r[use].reshape(-1)
        H += Jf.T @ Jf
        absH += np.abs(Jf).T @ np.abs(Jf)
        cost += float(rf @ rf)
        n += int(use.sum())
    return {"H": H, "cost": cost, "n": n, "absH": absH, "any_camera": any_camera}


def covariance(pose12, result, cams, sigma_px=None):
    """the definition -> dict(cov, info (6,6), stat (4,) = [ok, n, sigma_hat^2, min_pivot], and for the tolerances H, cost, absH, n, kappa =
    cond(D^-1/2 H D^-1/2)).  ok = 0: zero matrices, min_pivot 0."""
    zero = {"cov": np.zeros((6, 6)), "info": np.zeros((6, 6)), "kappa": np.inf}
    if int(np.asarray(result).reshape(-1)[0]) == 0:
        return dict(zero, stat=np.zeros(4), H=np.zeros((6, 6)), cost=0.0, absH=np.zeros((6, 6)), n=0)
    ne = normal_equations(pose12, cams)
    H, cost, n = ne["H"], ne["cost"], ne["n"]
    dof = 2 * n - 6
    finite = bool(np.isfinite(H).all() and np.isfinite(cost))
    s_hat2 = cost / dof if (finite and ne["any_camera"] and dof > 0) else 0.0
    fail = dict(zero, stat=np.array([0.0, n, s_hat2, 0.0]), **{k: ne[k] for k in ("H", "cost", "absH", "n")})
    s2 = float(sigma_px) ** 2 if sigma_px is not None else s_hat2
    if not (ne["any_camera"] and finite and (sigma_px is not None or dof > 0) and s2 > 0.0 and (np.diag(H) > 0).all()):
        return fail
    d = 1.0 / np.sqrt(np.diag(H))
    Hs = H * d[:, None] * d[None, :]
    Hs[np.arange(6), np.arange(6)] = 1.0
    L, min_pivot = np.zeros((6, 6)), 1.0
    for j in range(6):
        s = 1.0 - float(L[j, :j] @ L[j, :j])
        if not s > PIVOT_MIN:
            return fail
        min_pivot = min(min_pivot, s)
        L[j, j] = np.sqrt(s)
        for i in range(j + 1, 6):
            L[i, j] = (Hs[i, j] - float(L[i, :j] @ L[j, :j])) / L[j, j]
    Li = np.linalg.inv(L)
    Hinv = (Li.T @ Li) * d[:, None] * d[None, :]
    cov, info = s2 * 0.5 * (Hinv + Hinv.T), H / s2
    if not (np.isfinite(cov).all() and np.isfinite(info).all()):
        return fail
    return {"cov": cov, "info": info, "stat": np.array([1.0, n, s_hat2, min_pivot]), "kappa": float(np.linalg.cond(Hs)), "H": H, "cost": cost,
            "absH": ne["absH"], "n": n}


def frame_cam(X, uv, K4, mask=None):
    X = np.asarray(X, np.float64).reshape(-1, 3)
    return {"X": X, "uv": np.asarray(uv, np.float64).reshape(-1, 2), "K4": tuple(K4), "mask": np.ones(len(X), bool) if mask is None else mask}


def rig_cams(Xs, uvs, K4s, Es, masks=None):
    return [dict(frame_cam(X, uv, K4, None if masks is None else masks[c]), E=np.asarray(Es[c], np.float64)) for c, (X, uv, K4) in
            enumerate(zip(Xs, uvs, K4s))]


# ------------------------------------------------------------------------------------------------ tolerances (derived, ISSUE / DESIGN.md)
def bound_sums(ref):
    """entrywise bound of the difference of two summation orders of H (and, as a relative figure times cost, of cost):
    (2 n + 64) u sum_k |J_ki| |J_kj|"""
    return (2 * ref["n"] + 64) * U * ref["absH"]


def bound_matrix(ref, M):
    """entrywise bound for cov and info: 16 kappa (2 n + 64) u sqrt(M_ii M_jj)"""
    dg = np.sqrt(np.abs(np.diag(M)))
    return 16.0 * ref["kappa"] * (2 * ref["n"] + 64) * U * dg[:, None] * dg[None, :]


# ------------------------------------------------------------------------------------------------ NEES, transport
def so3_log(M):
    a = 0.5 * np.array([M[2, 1] - M[1, 2], M[0, 2] - M[2, 0], M[1, 0] - M[0, 1]])
    sn, cs = float(np.sqrt(a @ a)), 0.5 * (np.trace(M) - 1.0)
    th = np.arctan2(sn, cs)
    return a * (th / sn if sn > 1e-12 else 1.0)


def tangent_error(pose12, P_gt):
    """e = (omega, v) with exp(omega) R_est = R_gt, exp(omega) t_est + v = t_gt"""
    p = np.asarray(pose12, np.float64).reshape(12)
    R, t = p[:9].reshape(3, 3), p[9:]
    P_gt = np.asarray(P_gt, np.float64)
    w = so3_log(P_gt[:3, :3] @ R.T)
    Rn, tn = po.se3_update(np.eye(3), t, np.concatenate([w, np.zeros(3)]))
    return np.concatenate([w, P_gt[:3, 3] - tn])


def nees(pose12, P_gt, info, stat):
    if stat[0] == 0:
        return np.nan
    e = tangent_error(pose12, P_gt)
    return float(e @ info @ e)


def skew(t):
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0.0]])


def transport(cov, E):
    """the covariance of E o T from that of T: A cov A^T, A = [[R_c, 0], [[t_c]x R_c, R_c]]"""
    Rc, tc = np.asarray(E, np.float64)[:3, :3], np.asarray(E, np.float64)[:3, 3]
    A = np.zeros((6, 6))
    A[:3, :3], A[3:, 3:], A[3:, :3] = Rc, Rc, skew(tc) @ Rc
    return A @ cov @ A.T


def sigmas(cov):
    return float(np.degrees(np.sqrt(np.trace(cov[:3, :3])))), float(np.sqrt(np.trace(cov[3:, 3:])))


# ------------------------------------------------------------------------------------------------ scenes
CAL_K4 = (400.0, 400.0, 128.0, 40.0)
CAL_TRIALS, CAL_N, CAL_SEED = 64, 200, 0


def rotvec_matrix(w):
    return po.se3_update(np.eye(3), np.zeros(3), np.concatenate([w, np.zeros(3)]))[0]


def calibration_trial(rng, n=CAL_N, noise=1.0):
    """one trial of the calibration scene -> (X, uv float32-rounded float64, (R, t) truth)"""
    X = np.stack([rng.uniform(-20, 20, n), rng.uniform(-2, 2, n), rng.uniform(5, 40, n)], 1)
    R, t = rotvec_matrix(rng.uniform(-0.1, 0.1, 3)), rng.uniform(-1, 1, 3)
    X = rr.r32(X)
    uv, z = po.project(R, t, X, CAL_K4)
    assert (z > 1.0).all()
    return X, rr.r32(uv + rng.normal(size=(n, 2)) * noise), (R, t)


_cal = {}


def calibration_scene(n=CAL_N, trials=CAL_TRIALS, seed=CAL_SEED):
    """the trials of the calibration scene, computed once and never modified: list of (X, uv, truth)"""
    if (n, trials, seed) not in _cal:
        rng = np.random.default_rng(seed)
        _cal[n, trials, seed] = [calibration_trial(rng, n) for _ in range(trials)]
    return _cal[n, trials, seed]


def pose12_f32(R, t):
    """the pose as the solver stores it: rounded once to float32"""
    return rr.r32(np.concatenate([np.asarray(R).reshape(9), np.asarray(t).reshape(3)]))


FRAME_K4 = (700.0, 690.0, 256.0, 80.0)


def frame_scene(gen_seed, n, cap, outliers=0.3, noise=0.5, K4=FRAME_K4):
    """n valid rows in a capacity of `cap` (the rest finite junk nothing may read), int(outliers n) of them gross outliers; the points are
    drawn in front of the camera through the frustum -> (X (cap,3), uv (cap,2) float32, (R, t) truth)"""
    rng = np.random.default_rng(gen_seed)
    fx, fy, cx, cy = K4
    R, t = rotvec_matrix(rng.normal(size=3) * 0.3), rng.normal(size=3) * 2
    px = np.stack([rng.uniform(0, rr.W, n), rng.uniform(0, rr.H_IMG, n)], 1)
    depth = rng.uniform(6.0, 30.0, n)
    Y = np.stack([(px[:, 0] - cx) / fx * depth, (px[:, 1] - cy) / fy * depth, depth], 1)
    X = (Y - t) @ R
    uv = px + rng.normal(size=(n, 2)) * noise
    n_out = int(outliers * n)
    out = rng.permutation(n)[:n_out]
    uv[out] = np.stack([rng.uniform(0, rr.W, n_out), rng.uniform(0, rr.H_IMG, n_out)], 1)
    Xc = rng.uniform(-50, 50, (cap, 3)).astype(np.float32)
    uvc = rng.uniform(0, 512, (cap, 2)).astype(np.float32)
    Xc[:n], uvc[:n] = X, uv
    return Xc, uvc, (R, t)


def K_of(K4):
    return np.array([[K4[0], 0, K4[2]], [0, K4[1], K4[3]], [0, 0, 1.0]])
