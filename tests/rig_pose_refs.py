"""Float64 numpy restatement (TEST INFRASTRUCTURE ONLY) of the rig solver's definition ("Rig pose"; csrc/pnp.hip,
cofi_pnp_ransac_rig), built on oracle/pnp_oracle.py, plus the rig scenes the CPU and the GPU tests share.

Conventions.  A pose is (R (3,3), t (3,)).  Extrinsics E[c] = (3,4) [R_c | t_c], camera <- rig: Y_cam = R_c Y_rig + t_c.  The rig pose
T is rig <- cloud; camera c sees the cloud through compose(E[c], T).  A rig's data are lists over its cameras: Xs[c] (n_c,3), uvs[c]
(n_c,2), K4s[c] = (fx, fy, cx, cy).

f32=True makes a function round where the kernel rounds (the slab row once, every composed camera pose once), so that winner and
masks can be compared with the device's; the default is float64 throughout, which at C = 1 with identity extrinsics IS
pnp_oracle.solve_pnp_ransac."""
import numpy as np

import pnp_oracle as po
from pnp_oracle import hash_u32, hypothesis, reproj_err2, sample4, se3_update  # noqa: F401  (sample4: re-exported for the tests)

IDENTITY_E = np.hstack([np.eye(3), np.zeros((3, 1))])


def r32(a):
    """rounded once to float32, widened again"""
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


# ------------------------------------------------------------------------------------------------ the definition
def usable(K4):
    return K4[0] > 0 and K4[1] > 0


def eligible_rows(counts, K4s):
    """rows of every camera that can be drawn: usable intrinsics and at least 4 rows; 0 otherwise"""
    return [int(n) if (n >= 4 and usable(k)) else 0 for n, k in zip(counts, K4s)]


def camera_draw(seed, hyp, rows):
    """the camera of hypothesis `hyp`: g = hash(seed, hyp, 4) % total falls into the cumulative range of an eligible camera"""
    total = sum(rows)
    if total == 0:
        return None
    g = hash_u32(seed, hyp, 4) % total
    for c, n in enumerate(rows):
        if g < n:
            return c
        g -= n
    raise AssertionError("unreachable")


def compose(E, T):
    """E o T: the pose camera <- cloud of a camera with extrinsics E under the rig pose T"""
    Rc, tc = E[:, :3], E[:, 3]
    return Rc @ T[0], Rc @ T[1] + tc


def compose_inverse(E, P):
    """E^-1 o P with the transpose as the inverse rotation: the rig pose of a camera pose P"""
    Rc, tc = E[:, :3], E[:, 3]
    return Rc.T @ P[0], Rc.T @ (P[1] - tc)


def rig_hypothesis(seed, hyp, Xs, uvs, K4s, Es):
    """the rig pose of hypothesis `hyp` (fp64, unrounded), or None"""
    rows = eligible_rows([len(X) for X in Xs], K4s)
    c = camera_draw(seed, hyp, rows)
    if c is None:
        return None
    Rt = hypothesis(seed, hyp, np.asarray(Xs[c], np.float64), np.asarray(uvs[c], np.float64), K4s[c])
    return None if Rt is None else compose_inverse(Es[c], Rt)


def camera_pose(E, T, f32):
    R, t = compose(E, T)
    return (r32(R), r32(t)) if f32 else (R, t)


def rig_score(T, Xs, uvs, K4s, Es, f32=False):
    """squared reprojection errors of every row of every scored camera (usable, >= 1 row) under the rig pose T: a list over the
    cameras, None for a camera that is not scored"""
    out = []
    for X, uv, K4, E in zip(Xs, uvs, K4s, Es):
        if len(X) < 1 or not usable(K4):
            out.append(None)
            continue
        R, t = camera_pose(E, T, f32)
        out.append(reproj_err2(R, t, np.asarray(X, np.float64), np.asarray(uv, np.float64), K4))
    return out


def rig_cost_and_normal(R, t, Xs, uvs, K4s, Es):
    """cost, J^T J, J^T r of the reprojection error of all cameras' rows with respect to a left-multiplied se(3) increment of the RIG pose:
    row of camera c: Y_c = R_c (R X + t) + t_c, J = d(pi)/dY_c . R_c . [-[Y_rig]x | I]"""
    H, g, cost = np.zeros((6, 6)), np.zeros(6), 0.0
    for X, uv, (fx, fy, cx, cy), E in zip(Xs, uvs, K4s, Es):
        if len(X) == 0:
            continue
        Rc, tc = E[:, :3], E[:, 3]
        Yr = X @ R.T + t
        Y = Yr @ Rc.T + tc
        x, y, z = Y[:, 0], Y[:, 1], Y[:, 2]
        r = np.stack([fx * x / z + cx - uv[:, 0], fy * y / z + cy - uv[:, 1]], 1)
        a = np.zeros((len(X), 2, 3))
        a[:, 0, 0], a[:, 0, 2] = fx / z, -fx * x / z ** 2
        a[:, 1, 1], a[:, 1, 2] = fy / z, -fy * y / z ** 2
        A = a @ Rc
        S = np.zeros((len(X), 3, 3))
        S[:, 0, 1], S[:, 0, 2] = Yr[:, 2], -Yr[:, 1]
        S[:, 1, 0], S[:, 1, 2] = -Yr[:, 2], Yr[:, 0]
        S[:, 2, 0], S[:, 2, 1] = Yr[:, 1], -Yr[:, 0]
        J = np.concatenate([A @ S, A], 2).reshape(-1, 6)
        rf = r.reshape(-1)
        H += J.T @ J
        g += J.T @ rf
        cost += float(rf @ rf)
    return cost, H, g


def refine_rig(R, t, Xs, uvs, K4s, Es, iters=20):
    """po.refine on the rig pose over the given rows of all cameras: same damping, acceptance and solve"""
    Xs, uvs = [np.asarray(X, np.float64).reshape(-1, 3) for X in Xs], [np.asarray(u, np.float64).reshape(-1, 2) for u in uvs]
    lam = 1e-3
    c, H, g = rig_cost_and_normal(R, t, Xs, uvs, K4s, Es)
    for _ in range(iters):
        d = np.linalg.solve(H + lam * np.diag(np.diag(H)) + 1e-12 * np.eye(6), -g)
        Rn, tn = se3_update(R, t, d)
        cn, Hn, gn = rig_cost_and_normal(Rn, tn, Xs, uvs, K4s, Es)
        if np.isfinite(cn) and cn < c:
            R, t, c, H, g, lam = Rn, tn, cn, Hn, gn, max(lam * 0.1, 1e-9)
        else:
            lam = min(lam * 10.0, 1e6)
    return R, t


def solve_rig(Xs, uvs, K4s, Es, iterations=10000, reproj_error=8.0, seed=0, refine_iters=20, f32=False):
    """-> (success, R, t, masks (list over the cameras), winning hypothesis, inliers per camera).  On failure: identity, zero masks, -1."""
    Xs, uvs = [np.asarray(X, np.float64).reshape(-1, 3) for X in Xs], [np.asarray(u, np.float64).reshape(-1, 2) for u in uvs]
    fail = (False, np.eye(3), np.zeros(3), [np.zeros(len(X), bool) for X in Xs], -1, [0] * len(Xs))
    if sum(eligible_rows([len(X) for X in Xs], K4s)) == 0:
        return fail
    thr2 = reproj_error ** 2
    best = (-1, -1, None)
    for h in range(iterations):
        T = rig_hypothesis(seed, h, Xs, uvs, K4s, Es)
        if T is None:
            continue
        if f32:
            T = (r32(T[0]), r32(T[1]))
        cnt = sum(int(np.sum(e <= thr2)) for e in rig_score(T, Xs, uvs, K4s, Es, f32) if e is not None)
        if cnt > best[0]:
            best = (cnt, h, T)
    if best[2] is None or best[0] < 4:
        return fail
    T = best[2]
    masks = [np.zeros(len(X), bool) if e is None else e <= thr2 for X, e in zip(Xs, rig_score(T, Xs, uvs, K4s, Es, f32))]
    R, t = refine_rig(T[0], T[1], [X[m] for X, m in zip(Xs, masks)], [u[m] for u, m in zip(uvs, masks)], K4s, Es, refine_iters)
    return True, R, t, masks, best[1], [int(m.sum()) for m in masks]


def pose_matrix(R, t):
    P = np.eye(4)
    P[:3, :3], P[:3, 3] = R, t
    return P


# ------------------------------------------------------------------------------------------------ scenes
W, H_IMG = 512.0, 160.0


def rig_K4(c):
    """camera c's intrinsics: exact in float32, different per camera"""
    return (700.0 + 8 * c, 700.0 - 4 * c, 256.0 + c, 80.0 - c)


def rot_y(a):
    return np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])


def rot_x(a):
    return np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])


def rig_extrinsics_around(C, rng):
    """C cameras spread around the vertical (y) axis of the rig, about 0.5 m from it, each tilted a little: (C,3,4) float64, exactly
    orthonormal up to fp64 rounding"""
    E = np.zeros((C, 3, 4))
    for c in range(C):
        yaw = 2 * np.pi * c / C + rng.uniform(-0.1, 0.1)
        Rc = rot_x(rng.uniform(-0.05, 0.05)) @ rot_y(-yaw)                 # camera <- rig
        centre = 0.5 * np.array([np.sin(yaw), 0.0, np.cos(yaw)]) + rng.uniform(-0.05, 0.05, 3)   # the camera in the rig frame
        E[c, :, :3], E[c, :, 3] = Rc, -Rc @ centre
    return E


def rig_scene(gen_seed, counts, noise=0.5, outliers=0.3, inliers=None, single=False):
    """A rig of C = len(counts) cameras with counts[c] matches each.  Every camera's points are drawn in front of THAT camera (a pixel
    and a depth of 6 - 30 m, carried back into the cloud through the true poses); pixel noise `noise`; round(outliers * n) rows of a
    camera (or n - inliers[c]) get a uniform pixel instead.  single=True: one camera with identity extrinsics.
    -> dict(Xs, uvs float64 lists, K4s, E (C,3,4) float64, T = (R, t) ground truth rig <- cloud, inl = true-inlier masks)"""
    from scipy.spatial.transform import Rotation

    rng = np.random.default_rng(gen_seed)
    C = len(counts)
    E = IDENTITY_E[None].copy() if single else rig_extrinsics_around(C, rng)
    R = Rotation.from_rotvec(rng.normal(size=3) * 0.4).as_matrix()
    t = rng.normal(size=3) * 2
    Xs, uvs, K4s, inl = [], [], [], []
    for c, n in enumerate(counts):
        fx, fy, cx, cy = K4 = rig_K4(c)
        px = np.stack([rng.uniform(0, W, n), rng.uniform(0, H_IMG, n)], 1)
        depth = rng.uniform(6.0, 30.0, n)
        Yc = np.stack([(px[:, 0] - cx) / fx * depth, (px[:, 1] - cy) / fy * depth, depth], 1)
        Yr = (Yc - E[c, :, 3]) @ E[c, :, :3]              # R_c^T (Y_c - t_c)
        X = (Yr - t) @ R                                  # R^T (Y_r - t)
        uv = px + rng.normal(size=(n, 2)) * noise
        n_out = n - inliers[c] if inliers is not None else int(round(outliers * n))
        out = np.zeros(n, bool)
        out[rng.permutation(n)[:n_out]] = True
        uv[out] = np.stack([rng.uniform(0, W, n_out), rng.uniform(0, H_IMG, n_out)], 1)
        Xs.append(X), uvs.append(uv), K4s.append(K4), inl.append(~out)
    return {"Xs": Xs, "uvs": uvs, "K4s": K4s, "E": E, "T": (R, t), "inl": inl, "counts": tuple(counts)}


def as_f32(sc):
    """the scene as the device sees it: points, pixels and extrinsics rounded to float32 (widened again); the truth stays"""
    out = dict(sc)
    out["Xs"], out["uvs"], out["E"] = [r32(X) for X in sc["Xs"]], [r32(u) for u in sc["uvs"]], r32(sc["E"])
    return out


def rig_errors(R, t, T_true):
    """(RTE, RRE) of a rig pose against the truth, as the evaluation measures poses"""
    return po.get_P_diff(pose_matrix(R, t), pose_matrix(*T_true))


# name -> (generator seed, counts, noise, outlier share, inliers per camera or None, single camera with identity extrinsics).
# The starved rigs are the rows of the table in DESIGN.md: cameras with 2, 3 or 0 rows, and a rig none of whose cameras has 4 inliers.
SCENES = {
    "one_a": (11, (100,), 0.5, 0.3, None, True),
    "one_b": (12, (37,), 1.0, 0.3, None, True),
    "two_a": (21, (60, 37), 0.5, 0.3, None, False),
    "two_b": (22, (5, 90), 0.5, 0.3, None, False),
    "starved": (31, (40, 2, 3), 0.5, 0.3, (28, 2, 3), False),
    "even": (32, (30, 30, 30), 0.5, 0.3, None, False),
    "clean": (33, (30, 20, 14), 0.0, 0.0, None, False),
    "thin": (43, (5, 6, 4, 5), 0.5, 0.3, (3, 3, 3, 2), False),
    "thin_b": (42, (7, 4, 4, 6), 0.5, 0.3, (4, 3, 3, 3), False),
    "six": (61, (12, 9, 3, 20, 0, 7), 0.5, 0.3, None, False),
    "six_b": (62, (20, 20, 20, 20, 20, 20), 0.5, 0.3, None, False),
}
# the GPU runs: S = 2 rigs of equal C each; rig s is solved with seed SEED + s
SEED, ITERS = 7, 512
GPU_RUNS = {"C1": ("one_a", "one_b"), "C2": ("two_a", "two_b"), "C3": ("starved", "even"), "C3clean": ("clean", "even"),
            "C4": ("thin", "thin_b"), "C6": ("six", "six_b")}
ULP1 = float(np.spacing(np.float32(1.0)))

_scenes, _hyp = {}, {}


def scene(name):
    """the float32-rounded scene `name` (computed once, shared, never modified)"""
    if name not in _scenes:
        s, counts, noise, outl, inl, single = SCENES[name]
        _scenes[name] = as_f32(rig_scene(s, counts, noise, outl, inl, single))
    return _scenes[name]


def scene_hypotheses(name, seed, scale=1.0):
    """rig_hypothesis of all ITERS hypotheses of a scene (its pixels scaled by `scale`), computed once"""
    if (name, seed, scale) not in _hyp:
        sc = scene(name)
        uvs = [u * scale for u in sc["uvs"]]
        with np.errstate(all="ignore"):
            _hyp[name, seed, scale] = [rig_hypothesis(seed, h, sc["Xs"], uvs, sc["K4s"], sc["E"]) for h in range(ITERS)]
    return _hyp[name, seed, scale]


def stage1_differs(ref, got):
    """the stage-1 tolerance of tests/test_pose_stages_gpu.py between two poses: |dR| > 4 float32 ulp of 1 or |dt| > 4 ulp of max |t|"""
    dR = float(np.abs(np.asarray(got[0]) - ref[0]).max())
    dt = float(np.abs(np.asarray(got[1]) - ref[1]).max() / np.spacing(np.float32(np.abs(ref[1]).max())))
    return dR > 4 * ULP1 or dt > 4, dR, dt
