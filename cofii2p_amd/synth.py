"""Synthetic KITTI-shaped frames — there is no dataset access.

Host-side numpy only.  A frame mimics what `data/kitti.py:259-303` hands to the model:
a (3,H,W) image in [0,1), a voxel-lattice point cloud of exactly ``num_points`` points in the
camera frame (x right, y down, z forward) after a random yaw / in-plane shift
(`data/options.py:33-38`), and per-point features [intensity, nx, ny, nz] (`kitti.py:293`).
"""
from dataclasses import dataclass

import numpy as np


@dataclass
class Frame:
    img: np.ndarray  # (3,H,W) float32
    points: np.ndarray  # (N,3) float32
    feats: np.ndarray  # (N,4) float32
    seed: int


def make_frame(frame_id: int = 0, num_points: int = 20480, img_hw=(160, 512), extent: float = 40.0) -> Frame:
    seed = 1234 + int(frame_id)
    g = np.random.default_rng(seed)
    H, W = img_hw
    img = g.random((3, H, W), dtype=np.float32)

    n_raw = int(num_points * 1.6)
    n_ground = int(0.7 * n_raw)
    n_fac = n_raw - n_ground
    # ground plane 1.65 m below the camera (y is down)
    gx = g.uniform(-extent, extent, n_ground)
    gz = g.uniform(-extent, extent, n_ground)
    gy = 1.65 + g.normal(0.0, 0.03, n_ground)
    ground = np.stack([gx, gy, gz], 1)
    g_normal = np.tile(np.array([0.0, -1.0, 0.0]), (n_ground, 1))
    # 8 vertical facades, each with x or z fixed
    fac_pts, fac_nrm = [], []
    per = n_fac // 8
    for f in range(8):
        cnt = per if f < 7 else n_fac - 7 * per
        fixed = g.uniform(-extent + 5, extent - 5)
        u = g.uniform(-extent, extent, cnt)
        h = g.uniform(-6.0, 1.65, cnt)
        if f % 2 == 0:
            fac_pts.append(np.stack([np.full(cnt, fixed), h, u], 1))
            fac_nrm.append(np.tile(np.array([1.0, 0.0, 0.0]), (cnt, 1)))
        else:
            fac_pts.append(np.stack([u, h, np.full(cnt, fixed)], 1))
            fac_nrm.append(np.tile(np.array([0.0, 0.0, 1.0]), (cnt, 1)))
    pts = np.concatenate([ground] + fac_pts, 0)
    nrm = np.concatenate([g_normal] + fac_nrm, 0)
    # voxel lattice 0.1 m + de-duplication (mimics voxel_down_sample(0.1), kitti.py:283)
    pts = np.round(pts / 0.1) * 0.1
    _, first = np.unique(np.round(pts / 0.1).astype(np.int64), axis=0, return_index=True)
    first.sort()
    pts, nrm = pts[first], nrm[first]
    # resample to exactly num_points (kitti.py:168-180 downsample_np)
    if pts.shape[0] >= num_points:
        pick = g.choice(pts.shape[0], num_points, replace=False)
    else:
        pick = np.concatenate([np.arange(pts.shape[0]), g.choice(pts.shape[0], num_points - pts.shape[0], replace=True)])
    pts, nrm = pts[pick], nrm[pick]
    # random yaw about y and x/z shift (options.py:33-38)
    yaw = g.uniform(0.0, 2 * np.pi)
    c, s = np.cos(yaw), np.sin(yaw)
    R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    t = np.array([g.uniform(-10, 10), 0.0, g.uniform(-10, 10)])
    pts = pts @ R.T + t
    nrm = nrm @ R.T + g.normal(0.0, 0.05, nrm.shape)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    inten = g.random((num_points, 1))
    feats = np.concatenate([inten, nrm], 1)
    return Frame(img, pts.astype(np.float32), feats.astype(np.float32), seed)


def subsample_indices(n: int, num_stages: int, seed: int):
    """Index lists of the random half sub-sampling WITH replacement
    (preprocess_data.py:55-59), stage i+1 from stage i."""
    g = np.random.RandomState(seed)
    out = []
    for _ in range(num_stages - 1):
        out.append(g.choice(np.arange(n), size=n // 2))
        n //= 2
    return out


# KITTI odometry calibration of sequence 09 / 10 as data/kitti.py:24-63 reads it from calib.txt ("P2: ..." 3x4 projection row,
# "Tr: ..." velodyne -> camera 0), rounded values of the public calibration files
KITTI_CALIB_LINES = {
    "P0": "7.070912000000e+02 0.000000000000e+00 6.018873000000e+02 0.000000000000e+00 0.000000000000e+00 7.070912000000e+02 1.831104000000e+02 0.000000000000e+00 0.000000000000e+00 0.000000000000e+00 1.000000000000e+00 0.000000000000e+00",
    "P2": "7.070912000000e+02 0.000000000000e+00 6.018873000000e+02 4.688783000000e+01 0.000000000000e+00 7.070912000000e+02 1.831104000000e+02 1.178601000000e-01 0.000000000000e+00 0.000000000000e+00 1.000000000000e+00 6.203223000000e-03",
    "P3": "7.070912000000e+02 0.000000000000e+00 6.018873000000e+02 -3.334597000000e+02 0.000000000000e+00 7.070912000000e+02 1.831104000000e+02 1.930130000000e+00 0.000000000000e+00 0.000000000000e+00 1.000000000000e+00 3.318498000000e-03",
    "Tr": "-1.857739385241e-03 -9.999659513510e-01 -8.039975204516e-03 -4.784029760483e-03 -6.481465826011e-03 8.051860151134e-03 -9.999466081774e-01 -7.337429464231e-02 9.999773098287e-01 -1.805528627661e-03 -6.496203536139e-03 -3.339968064433e-01",
}


def make_raw_scan(frame_id: int = 0, num_points: int = 120000, img_hw=(376, 1241)):
    """A raw frame as it lies on disk for data/kitti.py:262-279: `data` (7, N) float32 = [xyz | intensity | normal] in the velodyne
    frame (x forward, y left, z up), `img` (H, W, 3) uint8, `K` (3, 3) float64.  Ground plane + facades sampled along rotating
    beams, denser near the sensor like a real scan, so the 0.1 m voxel grid merges several points per voxel close in and keeps
    single points far out."""
    g = np.random.default_rng(977 + int(frame_id))
    H, W = img_hw
    img = g.integers(0, 256, (H, W, 3), dtype=np.uint8)
    n_ground = int(0.6 * num_points)
    # ground: range ~ 3..70 m with 1/r density, full azimuth
    r = np.exp(g.uniform(np.log(3.0), np.log(70.0), n_ground))
    az = g.uniform(-np.pi, np.pi, n_ground)
    ground = np.stack([r * np.cos(az), r * np.sin(az), -1.73 + g.normal(0.0, 0.02, n_ground)], 1)
    g_n = np.tile(np.array([0.0, 0.0, 1.0]), (n_ground, 1))
    pts, nrm = [ground], [g_n]
    n_fac = num_points - n_ground
    per = n_fac // 10
    for f in range(10):
        cnt = per if f < 9 else n_fac - 9 * per
        d = g.uniform(5.0, 45.0) * (1 if f % 4 < 2 else -1)
        u = g.uniform(-50.0, 50.0, cnt) * g.uniform(0.2, 1.0, cnt)
        h = g.uniform(-1.73, 4.0, cnt)
        if f % 2 == 0:
            pts.append(np.stack([np.full(cnt, d) + g.normal(0, 0.02, cnt), u, h], 1))
            nrm.append(np.tile(np.array([-np.sign(d), 0.0, 0.0]), (cnt, 1)))
        else:
            pts.append(np.stack([u, np.full(cnt, d) + g.normal(0, 0.02, cnt), h], 1))
            nrm.append(np.tile(np.array([0.0, -np.sign(d), 0.0]), (cnt, 1)))
    pts = np.concatenate(pts, 0)
    nrm = np.concatenate(nrm, 0) + g.normal(0.0, 0.05, (num_points, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    inten = g.random((num_points, 1)) * 0.99
    order = g.permutation(num_points)
    data = np.concatenate([pts, inten, nrm], 1)[order].T.astype(np.float32)
    K = np.array([[707.0912, 0.0, 601.8873], [0.0, 707.0912, 183.1104], [0.0, 0.0, 1.0]])
    return np.ascontiguousarray(data), img, K


def make_raw_nuscenes(frame_id: int = 0, num_points: int = 26000, img_hw=(900, 1600)):
    """A nuScenes-style sample as data/nuscenes.py:183-193 reads it: `pc` (4, N) float32 = [xyz | intensity] ALREADY in the camera
    frame (x right, y down, z forward), `img` (H, W, 3) uint8, `K` (3, 3) float64."""
    g = np.random.default_rng(4242 + int(frame_id))
    H, W = img_hw
    img = g.integers(0, 256, (H, W, 3), dtype=np.uint8)
    n_ground = int(0.65 * num_points)
    r = np.exp(g.uniform(np.log(2.5), np.log(60.0), n_ground))
    az = g.uniform(-np.pi, np.pi, n_ground)
    ground = np.stack([r * np.sin(az), 1.8 + g.normal(0.0, 0.03, n_ground), r * np.cos(az)], 1)
    n_wall = num_points - n_ground
    u = g.uniform(-40.0, 40.0, n_wall)
    side = g.integers(0, 4, n_wall)
    d = g.uniform(8.0, 35.0, 4)[side]
    h = g.uniform(-5.0, 1.8, n_wall)
    wall = np.where((side % 2 == 0)[:, None], np.stack([np.where(side == 0, d, -d), h, u], 1), np.stack([u, h, np.where(side == 1, d, -d)], 1))
    pts = np.concatenate([ground, wall], 0)[g.permutation(num_points)]
    inten = g.uniform(0.0, 255.0, (num_points, 1))
    K = np.array([[1266.417, 0.0, 816.267], [0.0, 1266.417, 491.507], [0.0, 0.0, 1.0]])
    return np.ascontiguousarray(np.concatenate([pts, inten], 1).T.astype(np.float32)), img, K


def _quat_wxyz(yaw=0.0, pitch=0.0, roll=0.0):
    """unit quaternion (w, x, y, z) of Rz(yaw) Ry(pitch) Rx(roll)"""
    cy, sy, cp, sp, cr, sr = np.cos(yaw / 2), np.sin(yaw / 2), np.cos(pitch / 2), np.sin(pitch / 2), np.cos(roll / 2), np.sin(roll / 2)
    return np.array([cr * cp * cy + sr * sp * sy, sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy])


def _quat_matrix(q):
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def make_raw_sweeps(frame_id: int = 0, sweeps: int = 7, points_per_sweep: int = 34700, img_hw=(900, 1600), ld: int = 5, blind_first: bool = False):
    """One raw nuScenes-style sample as data/build_nuscenes/build_dataset.py:109-185, 239-268 reads it from the devkit: `sweeps` lidar
    sweeps, the key sweep first, then those the accumulation walk picks (later ones, then earlier ones), each (n, ld) float32 rows
    [x y z intensity (ring)] in ITS OWN lidar frame (x right, y forward, z up), taken from a vehicle that drives along the world's x axis -
    2 m between picked sweeps, a little yaw - over one shared scene (ground plane, four long facades), so the sweeps align once they are
    brought into the key sweep's frame.  The ground is sampled with 1 / r density from 0.5 m on: some points of every sweep fall into the
    ego box |x| < 0.8, |y| < 2.7.  Poses are (quaternion wxyz, translation) records as the devkit stores them.
    Returns {"sweeps": [...], "ego_poses": [(q, t)] per sweep, "lidar_calib": (q, t), "cameras": [{"img" (H, W, 3) uint8, "K" (3, 3)
    float32, "ego_pose": (q, t), "calib": (q, t)}]}: the front camera at the key sweep's time and once more 0.25 m further on; with
    blind_first a camera that looks away from the whole scene comes first, so that the in-picture threshold rejects it."""
    g = np.random.default_rng(31337 + int(frame_id))
    H, W = img_hw
    lidar_calib = (_quat_wxyz(yaw=-np.pi / 2), np.array([0.94, 0.0, 1.84]))       # lidar y = vehicle x (forward)
    cam_calib = (np.array([0.5, -0.5, 0.5, -0.5]), np.array([1.70, 0.01, 1.51]))  # camera z = vehicle x, camera x = vehicle -y, camera y = vehicle -z
    R_vl = _quat_matrix(lidar_calib[0])
    later = sweeps // 2                                        # 7 sweeps: the key sweep, 3 later, 3 earlier
    steps = [0] + list(range(1, later + 1)) + [-k for k in range(1, sweeps - later)]
    walls = [(0, 14.0), (0, -11.0), (1, 38.0), (1, -33.0)]     # (axis the facade is normal to: 0 = world y, 1 = world x; offset)
    out, poses = [], []
    for step in steps:
        yaw = 0.004 * step + g.normal(0.0, 0.001)
        pos = np.array([2.0 * step + g.normal(0.0, 0.02), 0.05 * step, 0.0])
        q = _quat_wxyz(yaw=yaw)
        R_wv = _quat_matrix(q)
        sensor = pos + R_wv @ lidar_calib[1]
        n_ground = int(0.6 * points_per_sweep)
        r = np.exp(g.uniform(np.log(0.5), np.log(70.0), n_ground))
        az = g.uniform(-np.pi, np.pi, n_ground)
        ground = np.stack([sensor[0] + r * np.cos(az), sensor[1] + r * np.sin(az), g.normal(0.0, 0.02, n_ground)], 1)
        n_wall = points_per_sweep - n_ground
        side = g.integers(0, 4, n_wall)
        u = g.uniform(-60.0, 60.0, n_wall) * g.uniform(0.15, 1.0, n_wall)
        h = g.uniform(0.0, 7.0, n_wall)
        off = np.array([w[1] for w in walls])[side] + g.normal(0.0, 0.02, n_wall)
        across = np.array([w[0] for w in walls])[side] == 0
        wall = np.where(across[:, None], np.stack([sensor[0] + u, off, h], 1), np.stack([off, sensor[1] + u, h], 1))
        world = np.concatenate([ground, wall], 0)[g.permutation(points_per_sweep)]
        veh = (world - pos) @ R_wv               # R_wv^T (world - pos)
        lid = (veh - lidar_calib[1]) @ R_vl
        cols = [lid, g.uniform(0.0, 255.0, (points_per_sweep, 1))]
        if ld == 5:
            cols.append(g.integers(0, 32, (points_per_sweep, 1)).astype(np.float64))
        out.append(np.ascontiguousarray(np.concatenate(cols, 1).astype(np.float32)))
        poses.append((q, pos))
    K = np.array([[1266.417, 0.0, 816.267], [0.0, 1266.417, 491.507], [0.0, 0.0, 1.0]], dtype=np.float32)
    cams = []
    if blind_first:
        cams.append({"img": g.integers(0, 256, (H, W, 3), dtype=np.uint8), "K": K.copy(), "ego_pose": (_quat_wxyz(yaw=np.pi), np.array([-300.0, 0.0, 0.0])),
                     "calib": cam_calib})
    for dx in (0.0, 0.25):
        cams.append({"img": g.integers(0, 256, (H, W, 3), dtype=np.uint8), "K": K.copy(), "ego_pose": (poses[0][0], poses[0][1] + np.array([dx, 0.0, 0.0])),
                     "calib": cam_calib})
    return {"sweeps": out, "ego_poses": poses, "lidar_calib": lidar_calib, "cameras": cams}
