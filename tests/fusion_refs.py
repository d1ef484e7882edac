"""A float64 numpy restatement of cofi_fuse_cloud_image (include/cofi_hip.h, "Registered clouds") and the scenes its tests run on.

fuse_ref: projection, z-buffer with splat, visibility gate, camera choice, bilinear colour, stats - the contract, in float64 on the
float32 operands (the intrinsics are the fp32 products K * k_scale the kernel forms, taken as inputs).

Scenes (make_scene): per cloud a jittered near wall that covers the middle of the picture in front of a far scatter (occlusion really
happens), a tenth of the points behind the camera, points outside the picture, points aimed at the border pixels, one NaN point, one
failed image (result = 0) when there are two or more, small random poses (further cameras of a cloud are yawed so that they see other
parts), smooth images (ramps plus low-frequency sines), K stored at half resolution and used with k_scale = 2.

The generator REMOVES (parks behind every camera, so that N is kept) each point whose answer fp32 could legitimately flip (unstable):
    u or v within 1e-3 px of a rounding boundary k + 1/2 (the picture's edges -1/2 and W - 1/2 are such boundaries),
    z within 1e-3 of z_near,
    z within 1e-3 max(1, z) of its gate zmin (1 + rel_tol) + abs_tol,
    z within 1e-4 relative of the minimum of a pixel it covers without being that minimum (an exact duplicate of the minimum stays:
        the lower id wins by rule, in any arithmetic),
    two cameras that see it with centrality measures within 1e-4 of each other (the camera choice could flip),
and repeats until nothing changes, since a removed point alters the buffer.  At most 2 % of a scene's points may go
(tests/test_fusion_refs_cpu.py asserts it for every scene the GPU tests use).

The fp32 error bound of (u, v) - uv_bound - from the projection body's operation count, with e = 2^-24 (half an ulp, relative):
    x_c = fma(r2, Z, fma(r1, Y, fma(r0, X, t0))): three roundings, each at most e times a partial sum, and every partial sum is at most
          M_x = |t0| + |r0 X| + |r1 Y| + |r2 Z|                                    =>  |dx| <= 3 e M_x   (likewise M_y, M_z)
    q = x_c / z_c, one division; allowing it 2 e |q| (a division that is not correctly rounded stays inside), to first order
          |dq| <= (|dx| + |q| |dz|) / |z| + 2 e |q|
    u = fma(fx, q, cx): one rounding                                               =>  |du| <= fx |dq| + e |u|
    and the same for v with y_c, fy, cy.  The bound is multiplied by 1 + 1e-3 for the second-order terms.
The colour bound - color_bound - per point and channel: bilinear interpolation with edge clamp is continuous and piecewise linear with
slope at most G = the largest difference between adjacent pixels of that channel's image (horizontally or vertically), so moving the
sample point by (du, dv) moves the value by at most G (|du| + |dv|).  Interpolation rounding: ax = u - floor(u) is exact; 1 - ax, 1 - ay
and the weight products are three roundings (3 e relative on each weight), the sum w00 p00 -> three fmas is four roundings of partial sums
of at most max|p| (the weights add up to 1): at most 7 e max|p|, taken as 8 e max|p|.
    bound = G (|du| + |dv|) + 8 e max|p|"""
import functools

import numpy as np

E32 = 2.0 ** -24
DEFAULTS = dict(k_scale=2.0, z_near=0.5, rel_tol=0.02, abs_tol=0.05)


def intrinsics(K, k_scale):
    """(F,4) float64 [fx, fy, cx, cy]: the fp32 products the kernel forms"""
    K32 = np.asarray(K, dtype=np.float32)
    ks = np.float32(k_scale)
    return np.stack([K32[:, 0, 0] * ks, K32[:, 1, 1] * ks, K32[:, 0, 2] * ks, K32[:, 1, 2] * ks], 1).astype(np.float64)


def project(P, pose12, k4, z_near, H, W):
    """points (N,3), one pose [R row-major | t], [fx, fy, cx, cy] -> u, v, z, in-picture (float64; a NaN fails every comparison)"""
    P = np.asarray(P, dtype=np.float64)
    pose12 = np.asarray(pose12, dtype=np.float64)
    R, t = pose12[:9].reshape(3, 3), pose12[9:]
    with np.errstate(all="ignore"):
        Xc = P @ R.T + t
        z = Xc[:, 2]
        u = k4[0] * (Xc[:, 0] / z) + k4[2]
        v = k4[1] * (Xc[:, 1] / z) + k4[3]
        ru, rv = np.round(u), np.round(v)                     # ties to even
        inn = (z > z_near) & (ru >= 0) & (ru <= W - 1) & (rv >= 0) & (rv <= H - 1)
    return u, v, z, inn


def crop_mask(P_cam, K, H, W):
    """the mask of crop_pc_with_img (data/kitti_helper.py:178-184) restated: np.round of K X / z, 0 <= px <= W - 1, 0 <= py <= H - 1"""
    pix = np.asarray(K, dtype=np.float64) @ np.asarray(P_cam, dtype=np.float64).T
    pix = np.round(pix / pix[2:, :])
    return (pix[0] >= 0) & (pix[0] <= W - 1) & (pix[1] >= 0) & (pix[1] <= H - 1)


def zbuffer(u, v, z, inn, H, W, splat):
    """-> zmin (H,W) float64 (inf where empty), index (H,W) (-1 where empty), and the entries (pixel, point, z) that competed"""
    ids = np.nonzero(inn)[0]
    px, py = np.round(u[ids]).astype(np.int64), np.round(v[ids]).astype(np.int64)
    pix, pid = [], []
    for dy in range(-splat, splat + 1):
        for dx in range(-splat, splat + 1):
            x, y = px + dx, py + dy
            ok = (x >= 0) & (x <= W - 1) & (y >= 0) & (y <= H - 1)
            pix.append((y * W + x)[ok])
            pid.append(ids[ok])
    pix = np.concatenate(pix) if pix else np.zeros(0, np.int64)
    pid = np.concatenate(pid) if pid else np.zeros(0, np.int64)
    zz = z[pid]
    zmin, index = np.full(H * W, np.inf), np.full(H * W, -1, dtype=np.int64)
    order = np.lexsort((pid, zz, pix))                        # nearest first, lowest id among equal depths
    first = np.ones(order.size, dtype=bool)
    first[1:] = pix[order][1:] != pix[order][:-1]
    win = order[first]
    zmin[pix[win]], index[pix[win]] = zz[win], pid[win]
    return zmin.reshape(H, W), index.reshape(H, W), (pix, pid, zz)


def bilinear(img, u, v):
    """img (Ci,H,W) float64, sample points -> (n,Ci): pixel centres at integers, taps clamped to the edge"""
    Ci, H, W = img.shape
    x0, y0 = np.floor(u), np.floor(v)
    ax, ay = u - x0, v - y0
    xa, xb = np.clip(x0, 0, W - 1).astype(np.int64), np.clip(x0 + 1, 0, W - 1).astype(np.int64)
    ya, yb = np.clip(y0, 0, H - 1).astype(np.int64), np.clip(y0 + 1, 0, H - 1).astype(np.int64)
    w00, w01, w10, w11 = (1 - ax) * (1 - ay), ax * (1 - ay), (1 - ax) * ay, ax * ay
    return (w00 * img[:, ya, xa] + w01 * img[:, ya, xb] + w10 * img[:, yb, xa] + w11 * img[:, yb, xb]).T


def fuse_ref(points, images, pose, K, result=None, cameras=1, k_scale=1.0, z_near=0.5, splat=1, rel_tol=0.02, abs_tol=0.05):
    """The contract in float64.  points (S,N,3) float32, images (F,Ci,H,W) float32, pose (F,12), K (F,3,3), result (F,) or None.
    -> dict of the six outputs (depth as float64) plus u, v, z (F,N), r2 (F,N), zmin (F,H,W) and the unstable mask (S,N) of the docstring."""
    points, images = np.asarray(points), np.asarray(images, dtype=np.float64)
    S, N, _ = points.shape
    F, Ci, H, W = images.shape
    C = cameras
    assert F == S * C
    k4 = intrinsics(K, k_scale)
    ok = np.ones(F, dtype=bool) if result is None else np.asarray(result).reshape(F, -1)[:, 0] != 0
    U, V, Z = np.zeros((F, N)), np.zeros((F, N)), np.zeros((F, N))
    INN, VIS = np.zeros((F, N), dtype=bool), np.zeros((F, N), dtype=bool)
    zmin_all, depth, index = np.full((F, H, W), np.inf), np.zeros((F, H, W)), np.full((F, H, W), -1, dtype=np.int32)
    unstable = np.zeros((S, N), dtype=bool)
    R2 = np.full((F, N), np.inf)
    for f in range(F):
        s = f // C
        u, v, z, inn = project(points[s], pose[f], k4[f], z_near, H, W)
        U[f], V[f], Z[f] = u, v, z
        with np.errstate(all="ignore"):
            # the flip zone of the in-picture test (whatever the image's result: a superset)
            near = (z >= z_near - 1e-3) & (u >= -1) & (u <= W) & (v >= -1) & (v <= H)
            unstable[s] |= near & ((np.abs(u - np.floor(u) - 0.5) < 1e-3) | (np.abs(v - np.floor(v) - 0.5) < 1e-3) | (np.abs(z - z_near) <= 1e-3))
        zmin, idx, (pix, pid, zz) = zbuffer(u, v, z, inn, H, W, splat)
        zm = zmin.reshape(-1)[pix]
        close = (zz != zm) & (zz - zm <= 1e-4 * zm)
        unstable[s, pid[close]] = True
        ids = np.nonzero(inn)[0]
        own = zmin[np.round(v[ids]).astype(np.int64), np.round(u[ids]).astype(np.int64)]
        gate = own * (1.0 + rel_tol) + abs_tol
        unstable[s, ids[np.abs(z[ids] - gate) <= 1e-3 * np.maximum(1.0, z[ids])]] = True
        if not ok[f]:
            continue
        INN[f] = inn
        VIS[f, ids] = z[ids] <= gate
        zmin_all[f] = zmin
        depth[f] = np.where(idx >= 0, zmin, 0.0)
        index[f] = idx
        R2[f, VIS[f]] = ((u[VIS[f]] - k4[f, 2]) / k4[f, 0]) ** 2 + ((v[VIS[f]] - k4[f, 3]) / k4[f, 1]) ** 2
    camera = np.full((S, N), -1, dtype=np.int32)
    color = np.zeros((S, N, Ci))
    for s in range(S):
        r2 = R2[s * C:(s + 1) * C]                             # (C,N)
        best = np.argmin(r2, 0)                               # the first = lowest camera on ties
        seen = np.isfinite(r2[best, np.arange(N)])
        camera[s, seen] = best[seen]
        if C > 1:
            two = np.sort(r2, 0)[:2]
            with np.errstate(invalid="ignore"):
                unstable[s] |= np.isfinite(two[1]) & (two[1] - two[0] <= 1e-4)
        for c in range(C):
            m = seen & (best == c)
            color[s, m] = bilinear(images[s * C + c], U[s * C + c, m], V[s * C + c, m])
    flags = (INN.astype(np.uint8) | (VIS.astype(np.uint8) << 1)).astype(np.uint8)
    stats = np.stack([INN.sum(1), VIS.sum(1), (index >= 0).reshape(F, -1).sum(1), np.zeros(F, dtype=np.int64)], 1).astype(np.int32)
    return {"depth": depth, "index": index, "flags": flags, "color": color, "camera": camera, "stats": stats,
            "u": U, "v": V, "z": Z, "r2": R2, "zmin": zmin_all, "unstable": unstable, "k4": k4}


def uv_bound(P, pose12, k4):
    """(du, dv): the fp32 error bounds of the module docstring for points (n,3) under one pose"""
    P, pose12 = np.asarray(P, dtype=np.float64), np.asarray(pose12, dtype=np.float64)
    R, t = pose12[:9].reshape(3, 3), pose12[9:]
    M = np.abs(P) @ np.abs(R).T + np.abs(t)                    # (n,3): M_x, M_y, M_z
    Xc = P @ R.T + t
    z = np.abs(Xc[:, 2])
    out = []
    for a, (f_, c_) in enumerate(((k4[0], k4[2]), (k4[1], k4[3]))):
        q = np.abs(Xc[:, a]) / z
        dq = (3 * E32 * M[:, a] + q * 3 * E32 * M[:, 2]) / z + 2 * E32 * q
        out.append((f_ * dq + E32 * np.abs(f_ * Xc[:, a] / Xc[:, 2] + c_)) * (1 + 1e-3))
    return out[0], out[1]


def color_bound(scene, ref):
    """(S,N,Ci): the colour bound of the module docstring for every point (0 where unseen: the value is exactly 0 there)"""
    pts, images, pose = scene["points"], scene["images"].astype(np.float64), scene["pose"]
    S, N, _ = pts.shape
    F, Ci, H, W = images.shape
    C = scene["cameras"]
    G = np.zeros((F, Ci))
    for f in range(F):
        for ch in range(Ci):
            im = images[f, ch]
            G[f, ch] = max(np.abs(np.diff(im, axis=0)).max() if H > 1 else 0.0, np.abs(np.diff(im, axis=1)).max() if W > 1 else 0.0)
    pmax = np.abs(images).reshape(F, Ci, -1).max(2)
    out = np.zeros((S, N, Ci))
    for s in range(S):
        for c in range(C):
            f = s * C + c
            m = ref["camera"][s] == c
            du, dv = uv_bound(pts[s, m], pose[f], ref["k4"][f])
            out[s, m] = G[f][None, :] * (du + dv)[:, None] + 8 * E32 * pmax[f][None, :]
    return out


# ------------------------------------------------------------------------------------------------ scenes
def small_pose(rng, yaw=0.0):
    """[R | t] of a small random rotation (about 0.03 rad per axis) after a yaw, t of about 0.1"""
    w = rng.normal(scale=0.03, size=3) + np.array([0.0, yaw, 0.0])
    th = np.linalg.norm(w)
    Kx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    R = np.eye(3) + np.sin(th) / th * Kx + (1 - np.cos(th)) / th ** 2 * Kx @ Kx
    return np.concatenate([R.reshape(9), rng.normal(scale=0.1, size=3)])


def smooth_images(F, Ci, H, W):
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    out = np.zeros((F, Ci, H, W))
    for f in range(F):
        for ch in range(Ci):
            out[f, ch] = 0.3 + 0.2 * x / W + 0.1 * (ch + 1) * y / (H * Ci) + 0.2 * np.sin(2 * np.pi * (0.7 * x / W + 0.4 * y / H) + ch + 0.5 * f)
    return out.astype(np.float32)


def raw_scene(seed, N, H, W, S, C, Ci):
    """the scene before any removal (see the module docstring)"""
    rng = np.random.default_rng(seed)
    F = S * C
    K = np.zeros((F, 3, 3), dtype=np.float32)                  # half resolution: used with k_scale = 2
    for f in range(F):
        fx = 0.45 * W * (1 + 0.05 * rng.uniform(-1, 1))
        K[f] = [[fx, 0, (W - 1) / 4 + 0.1 * rng.uniform(-1, 1)], [0, fx * (1 + 0.02 * rng.uniform(-1, 1)), (H - 1) / 4 + 0.1 * rng.uniform(-1, 1)], [0, 0, 1]]
    k4 = intrinsics(K, 2.0)
    pose = np.zeros((F, 12))
    for f in range(F):
        c = f % C
        pose[f] = small_pose(rng, yaw=0.0 if c == 0 else (0.18 if c % 2 else -0.18) * ((c + 1) // 2))
    pose = pose.astype(np.float32)
    points = np.zeros((S, N, 3), dtype=np.float32)
    for s in range(S):
        kind = rng.uniform(size=N)
        kind[0] = 0.0                                         # point 0 is a wall point: a cloud of one point has something to show
        wall, behind, border = kind < 0.35, (kind >= 0.35) & (kind < 0.45), (kind >= 0.45) & (kind < 0.52)
        z = rng.uniform(5.0, 30.0, N)
        u, v = rng.uniform(-0.3 * W, 1.3 * W, N), rng.uniform(-0.3 * H, 1.3 * H, N)
        z[wall] = 3.0 + rng.uniform(-0.4, 0.4, wall.sum())
        u[wall], v[wall] = rng.uniform(0.15 * W, 0.85 * W, wall.sum()), rng.uniform(0.15 * H, 0.85 * H, wall.sum())
        z[behind] = rng.uniform(-30.0, -1.0, behind.sum())
        nb = int(border.sum())
        side = rng.integers(0, 4, nb)
        off = rng.uniform(-0.4, 0.4, nb)
        u[border] = np.where(side == 0, off, np.where(side == 1, W - 1 + off, u[border].clip(0, W - 1)))
        v[border] = np.where(side == 2, off, np.where(side == 3, H - 1 + off, v[border].clip(0, H - 1)))
        # the targets are pixels of the cloud's first camera: carried into the cloud frame through that camera's pose
        f0 = s * C
        cam = np.stack([z * (u - k4[f0, 2]) / k4[f0, 0], z * (v - k4[f0, 3]) / k4[f0, 1], z], 1)
        R, t = pose[f0, :9].astype(np.float64).reshape(3, 3), pose[f0, 9:].astype(np.float64)
        points[s] = ((cam - t) @ R).astype(np.float32)
        if N >= 8:
            points[s, N // 2, 0] = np.nan
    result = np.ones((F, 3), dtype=np.int32)
    result[:, 1:] = rng.integers(5, 50, (F, 2))
    if F >= 2:
        result[F - 1, 0] = 0                                  # one failed image
    return {"points": points, "images": smooth_images(F, Ci, H, W), "pose": pose, "K": K, "result": result, "cameras": C, "seed": seed}


def ref_of(scene, splat):
    return fuse_ref(scene["points"], scene["images"], scene["pose"], scene["K"], scene["result"][:, 0], scene["cameras"], splat=splat,
                    **DEFAULTS)


def condition(scene, splat):
    """park every unstable point behind all cameras until nothing changes -> the number of points removed"""
    pts = scene["points"]
    S, N, _ = pts.shape
    removed = np.zeros((S, N), dtype=bool)
    for _ in range(64):
        bad = ref_of(scene, splat)["unstable"]
        if not bad.any():
            break
        removed |= bad
        for s, i in zip(*np.nonzero(bad)):
            pts[s, i] = (0.01 * (i % 7), 0.0, -10.0 - 0.001 * i)
    else:
        raise AssertionError("the removal did not settle")
    scene["removed"] = int(removed.sum())
    return scene["removed"]


# (N, H, W, S, C, splat, Ci, seed): every value of every parameter the issue lists occurs; the seeds are the first for which the cap
# holds (decided by this file's float64 reference alone)
CASES = [
    (1, 5, 7, 1, 1, 0, 1, 0),
    (63, 5, 7, 3, 1, 1, 3, 0),
    (63, 16, 24, 1, 3, 2, 5, 0),
    (257, 16, 24, 2, 2, 0, 3, 0),
    (257, 5, 7, 1, 1, 2, 1, 0),
    (1000, 40, 64, 3, 1, 1, 5, 0),
    (1000, 16, 24, 1, 3, 0, 3, 0),
    (4099, 40, 64, 2, 2, 2, 3, 0),
    (4099, 40, 64, 1, 1, 1, 1, 0),
    (4099, 16, 24, 1, 3, 1, 5, 0),
]
CASE_IDS = ["N%d-%dx%d-S%dC%d-splat%d-Ci%d" % c[:7] for c in CASES]


@functools.lru_cache(maxsize=None)
def scene(case):
    """(conditioned scene, its reference): computed once, shared, never modified by the tests"""
    N, H, W, S, C, splat, Ci, seed = case
    sc = raw_scene(1000 * seed + 17 * N + H, N, H, W, S, C, Ci)
    condition(sc, splat)
    sc["splat"] = splat
    ref = ref_of(sc, splat)
    for a in list(sc.values()) + list(ref.values()):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return sc, ref
