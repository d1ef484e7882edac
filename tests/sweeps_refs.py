"""Plain numpy restatements of the raw-sweep path (cofii2p_amd/sweeps.py, csrc/dataside.hip): what data/build_nuscenes/build_dataset.py
does to one sample - ego-box cut and accumulation of the sweeps (:109-185), the 0.2 m voxel grid with reflectance (:41-54), the move into
the camera frame with the in-picture count (:265-280), crop and resize of the image (:252-260), and the three acceptance tests (:218,
:228, :291).  Written from the description of those lines, one numpy statement per floating-point operation, in the order the kernels
use, so the GPU tests compare bit for bit.  numpy never fuses a product with a sum, the library is built with -ffp-contract=off.

The devkit, pyquaternion, open3d and cv2 are absent: parity with open3d's map order and averaging, with cv2.resize and with pyquaternion
is unpinned.  tests/test_sweeps_refs_cpu.py holds these functions against np.dot, a dictionary voxel grid, oracle/dataside_oracle.py and
scipy."""
import numpy as np

F32 = np.float32
KEY_BITS = 13


def ego_keep(rows):
    """:115-121 on (n, ld) float32 rows: True where the point is NOT on the ego vehicle (strict float32 compares)"""
    x, y = rows[:, 0].astype(F32), rows[:, 1].astype(F32)
    inside = (x < F32(0.8)) & (x > F32(-0.8)) & (y < F32(2.7)) & (y > F32(-2.7))
    return ~inside


def affine64(M, p, translate=True):
    """(n, 3) float64 -> rows M[a, 0:3] . p (+ M[a, 3]): s = M[a,0] x; s = s + M[a,1] y; s = s + M[a,2] z; (s = s + M[a,3])"""
    M = np.asarray(M, np.float64)
    p = np.asarray(p, np.float64)
    out = np.empty((p.shape[0], 3), np.float64)
    for a in range(3):
        s = M[a, 0] * p[:, 0]
        s = s + M[a, 1] * p[:, 1]
        s = s + M[a, 2] * p[:, 2]
        if translate:
            s = s + M[a, 3]
        out[:, a] = s
    return out


def accumulate(sweeps, transforms):
    """:127-185: kept points of all sweeps in sweep order, then original order; sweep 0 widened as it is, sweep j > 0 through transforms[j].
    -> points (n, 3) float64, intensity (n,) float32"""
    pts, inten = [], []
    for j, sw in enumerate(sweeps):
        sw = np.asarray(sw, F32).reshape(-1, np.asarray(sw).shape[-1])
        kept = sw[ego_keep(sw)]
        p = kept[:, 0:3].astype(np.float64)
        pts.append(p if j == 0 else affine64(transforms[j], p))
        inten.append(kept[:, 3])
    return np.concatenate(pts, 0).reshape(-1, 3), np.concatenate(inten, 0).astype(F32)


def voxel_indices(points, voxel, minb=None):
    """open3d: floor((p - (min_bound - voxel / 2)) / voxel) per axis, in double"""
    points = np.asarray(points, np.float64)
    if minb is None:
        minb = points.min(0) - voxel * 0.5
    return np.floor((points - minb) / voxel).astype(np.int64), minb


def voxel_downsample(points, intensity, voxel=0.2):
    """:41-54 on float64 points (n, 3) and float32 intensity (n,) -> ((M, 4) float32 rows [xyz | intensity] in ascending key order, overflow).
    Keys of 13 bits per axis (clamped, overflow flagged); per-voxel sums in double in input order, times 1.0 / count; the colour is
    float32(intensity / max) widened, its mean times the widened max in double, cast last."""
    points = np.asarray(points, np.float64)
    intensity = np.asarray(intensity, F32)
    vidx, _ = voxel_indices(points, voxel)
    top = (1 << KEY_BITS) - 1
    overflow = bool(((vidx < 0) | (vidx > top)).any())
    vidx = np.clip(vidx, 0, top)
    key = (vidx[:, 0] << (2 * KEY_BITS)) | (vidx[:, 1] << KEY_BITS) | vidx[:, 2]
    order = np.argsort(key, kind="stable")
    sk = key[order]
    first = np.flatnonzero(np.concatenate([[True], sk[1:] != sk[:-1]]))
    count = np.diff(np.concatenate([first, [len(sk)]]))
    imax = intensity.max()
    colour = (intensity / imax).astype(F32).astype(np.float64)

    def means(values):
        v = values[order]
        total = np.zeros(len(first), np.float64)
        for step in range(int(count.max())):          # the step-th member of every voxel that has one: sequential sums
            sel = np.flatnonzero(count > step)
            total[sel] = total[sel] + v[first[sel] + step]
        return total * (1.0 / count.astype(np.float64))

    rows = np.empty((len(first), 4), F32)
    for a in range(3):
        rows[:, a] = means(points[:, a]).astype(F32)
    rows[:, 3] = (means(colour) * np.float64(imax)).astype(F32)
    return rows, overflow


def voxel_downsample_dict(points, intensity, voxel=0.2):
    """the same grid by brute force: a dictionary from voxel index to its members, Python float sums"""
    points = np.asarray(points, np.float64)
    intensity = np.asarray(intensity, F32)
    minb = points.min(0) - voxel * 0.5
    imax = intensity.max()
    cells = {}
    for i in range(points.shape[0]):
        idx = tuple(int(np.floor((points[i, a] - minb[a]) / voxel)) for a in range(3))
        cells.setdefault(idx, []).append(i)
    rows = []
    for idx in sorted(cells):
        acc = [0.0, 0.0, 0.0, 0.0]
        for i in cells[idx]:
            for a in range(3):
                acc[a] += float(points[i, a])
            acc[3] += float(F32(intensity[i] / imax))
        inv = 1.0 / float(len(cells[idx]))
        rows.append([F32(acc[0] * inv), F32(acc[1] * inv), F32(acc[2] * inv), F32((acc[3] * inv) * float(imax))])
    return np.asarray(rows, F32).reshape(-1, 4)


def to_camera(rows, P, K, hw):
    """:265-280: (M, 4) float32 rows -> ((4, M) float32 [float32(R p + t) | intensity], points in the picture).  P float64 4x4, K float32 3x3."""
    rows = np.asarray(rows, F32)
    H, W = hw
    c = affine64(P, rows[:, 0:3].astype(np.float64))
    uvz = affine64(np.asarray(K, F32).astype(np.float64), c, translate=False)
    depth = uvz[:, 2]
    front = depth > 0
    u, v = np.zeros_like(depth), np.zeros_like(depth)
    u[front] = uvz[front, 0] / depth[front]
    v[front] = uvz[front, 1] / depth[front]
    inside = front & (u >= 0) & (u <= W - 1) & (v >= 0) & (v <= H - 1)
    pc = np.concatenate([c.astype(F32).T, rows[:, 3][None, :]], 0)
    return np.ascontiguousarray(pc), int(inside.sum())


def resized_hw(hw, top, scale):
    """:256-258: (int(round(w s)), int(round(h s))) of the cropped image, Python round -> (h, w)"""
    return int(round((hw[0] - top) * scale)), int(round(hw[1] * scale))


def resize_u8(img, top, scale):
    """:252-260: cv2.resize(img[top:], INTER_LINEAR) on uint8 HWC in OpenCV's fixed-point arithmetic: 11-bit weights rounded half to even,
    the horizontal pass exact in integers, the vertical pass ((w0 * (r0 >> 4)) >> 16) + ((w1 * (r1 >> 4)) >> 16) + 2) >> 2"""
    src = np.asarray(img)[top:].astype(np.int64)
    sh, sw = src.shape[:2]
    dh, dw = resized_hw(img.shape[:2], top, scale)

    def taps(dn, sn):
        ratio = np.float64(F32(float(sn) / dn))
        pos = ((np.arange(dn) + 0.5) * ratio - 0.5).astype(F32)
        base = np.floor(pos).astype(np.int64)
        frac = pos - base.astype(F32)
        low, high = base < 0, base >= sn - 1
        frac[low | high] = 0
        base[low] = 0
        base[high] = sn - 1
        w1 = np.rint(frac * F32(2048)).astype(np.int64)
        w0 = np.rint((F32(1) - frac) * F32(2048)).astype(np.int64)
        return base, np.minimum(base + 1, sn - 1), w0, w1

    x0, x1, wx0, wx1 = taps(dw, sw)
    y0, y1, wy0, wy1 = taps(dh, sh)
    hor = src[:, x0] * wx0[None, :, None] + src[:, x1] * wx1[None, :, None]
    val = (((wy0[:, None, None] * (hor[y0] >> 4)) >> 16) + ((wy1[:, None, None] * (hor[y1] >> 4)) >> 16) + 2) >> 2
    return np.clip(val, 0, 255).astype(np.uint8)


def scaled_K(K, top, scale):
    """:254, :260: camera_matrix_cropping(K, 0, top) then camera_matrix_scaling(., scale), float32 throughout"""
    Kc = np.array(K, dtype=F32)
    Kc[1, 2] = Kc[1, 2] - F32(top)
    Ks = F32(scale) * Kc
    Ks[2, 2] = 1
    return Ks


def build_sample(sweeps, transforms, cameras, top=100, scale=0.4, min_points=45000, min_inside=6000, voxel=0.2):
    """make_dataset (:217-300) for one sample -> (dict or None, reason)"""
    pts, inten = accumulate(sweeps, transforms)
    if pts.shape[0] < min_points:
        return None, "accumulated"
    rows, overflow = voxel_downsample(pts, inten, voxel)
    assert not overflow
    if rows.shape[0] < min_points:
        return None, "voxels"
    for ci, (img, K, P) in enumerate(cameras):
        Ks = scaled_K(K, top, scale)
        hw = resized_hw(img.shape[:2], top, scale)
        pc, inside = to_camera(rows, P, Ks, hw)
        if inside > min_inside:
            return {"pc": pc, "img": resize_u8(img, top, scale), "K": Ks, "P": np.asarray(P, np.float64), "inside": inside,
                    "accumulated": int(pts.shape[0]), "voxels": int(rows.shape[0]), "camera": ci}, None
    return None, "inside"


def pose_matrix(rotation_wxyz, translation):
    """:68-88: unit quaternion (w, x, y, z) -> rotation matrix, rounded to float32 with the translation, placed into a float64 4x4"""
    q = np.asarray(rotation_wxyz, np.float64)
    w, x, y, z = q / np.sqrt(np.dot(q, q))
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    P = np.identity(4)
    P[0:3, 0:3] = R.astype(F32)
    P[0:3, 3] = np.asarray(translation, np.float64).astype(F32)
    return P


def boundary_cases(seed, candidates=4000000, voxel=0.2, reach=64.0):
    """Transformed points whose voxel index changes when they are rounded to float32 first.  A key-sweep anchor point fixes the minimum
    bound; random float32 points in a cube of `reach` metres go through a random rigid transform in double; those whose float64 index
    differs on some axis from the index of their float32 rounding are returned.
    -> (anchor (3,) float64 - float32-valued -, transform (4, 4) float64, raw (k, 3) float32, transformed (k, 3) float64,
        companions (k, 3) float32 raw points)"""
    g = np.random.default_rng(seed)
    anchor = np.array([-reach - 2.0, -reach - 2.0, -reach - 2.0]).astype(F32).astype(np.float64)
    ang = g.uniform(-np.pi, np.pi)
    T = np.identity(4)
    T[0:2, 0:2] = [[np.cos(ang), -np.sin(ang)], [np.sin(ang), np.cos(ang)]]
    T[0:3, 3] = g.uniform(-1.0, 1.0, 3)
    raw = g.uniform(-reach / 1.5, reach / 1.5, (candidates, 3)).astype(F32)
    raw = raw[ego_keep(raw)]
    moved = affine64(T, raw.astype(np.float64))
    minb = anchor - voxel * 0.5
    assert (moved.min(0) > anchor).all()
    exact, _ = voxel_indices(moved, voxel, minb)
    rounded, _ = voxel_indices(moved.astype(F32).astype(np.float64), voxel, minb)
    hit = np.flatnonzero((exact != rounded).any(1))
    # a companion per case at the centre of the case's float64 voxel: with exact keys the pair shares a voxel, with float32-rounded
    # points the case moves next door and the grid has one voxel more per case
    centre = minb + (exact[hit].astype(np.float64) + 0.5) * voxel
    mate = affine64(np.linalg.inv(T), centre).astype(F32)
    ok = ego_keep(mate)
    mate_idx, _ = voxel_indices(affine64(T, mate.astype(np.float64)), voxel, minb)
    ok &= (mate_idx == exact[hit]).all(1)
    hit, mate = hit[ok], mate[ok]
    return anchor, T, raw[hit], moved[hit], mate
