"""Raw nuScenes sweeps -> the stored sample `FramePreparer(dataset='nuscenes')` takes, on the device: what
data/build_nuscenes/build_dataset.py does per sample with open3d / numpy / cv2 on the host.

    key sweep + up to 3 later and 3 earlier sweeps  --ego-box cut, T_j in float64-->  accumulated cloud (float64) + reflectance
      --0.2 m voxel grid on the float64 points-->  (M, 4) float32 rows  --P_cam_pc, K-->  (4, M) cloud in the camera frame + in-picture count
    camera image (900, 1600, 3) uint8  --drop the top rows, x0.4 bilinear-->  (320, 640, 3) uint8

The kernels are in csrc/dataside.hip (cofi_accumulate_sweeps, cofi_voxel_downsample_f64, cofi_sweeps_to_camera, cofi_resize_image_u8);
tests/sweeps_refs.py restates them in numpy bit for bit.  The small matrix algebra (poses, which sweeps to take) is host numpy in
float64, written the way the reference writes it.

Unpinned, because the devkit, pyquaternion, open3d and cv2 are not available to the tests: open3d's voxel order (ascending voxel index
here) and averaging, cv2.resize, pyquaternion's rotation matrix.  The reference stores the cloud as float64 (:293-294 concatenates the
float64 camera-frame points with the float32 reflectance); this path hands float32 to the preparer, which converts to float32 on entry
anyway (cofii2p_amd/dataside.py).

The three acceptance tests of the reference (:218, :228, :291) are host decisions there and here: `build_sample` waits once on the
accumulated count, once on the voxel count and once per tried camera on the in-picture count (pinned copy + event).
"""
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib, ops

VOXEL_SIZE = 0.2          # build_dataset.py:224
MIN_POINTS = 45000        # :218, :228
MIN_INSIDE = 6000         # :291
TOP_ROWS = 100            # data/options.py:71 crop_original_top_rows
IMG_SCALE = 0.4           # data/options.py:72 img_scale
MAX_SWEEPS = 64


# ---------------------------------------------------------------------------------------------- host side: poses and picks
def accumulation_picks(available: int, num: int = 3, skip: int = 4) -> List[int]:
    """The walk of build_dataset.py:127-153 along one direction of the sweep chain: hop counts (1 = the sweep next to the key sweep)
    of the sweeps it accumulates when `available` sweeps follow the key sweep in that direction.  Defaults
    (data/options.py:68-69): 4, 8, 12, cut off by `available`."""
    picks = []
    counter, taken, here = 1, 0, 0     # `here`: hops of the sweep the walk stands on
    while taken < num:
        if here + 1 > available:       # lidar[direction] == ''
            break
        if counter % skip != 0:
            counter += 1
            here += 1
            continue
        picks.append(here + 1)
        counter += 1
        here += 1
        taken += 1
    return picks


def pose_matrix(rotation_wxyz, translation) -> np.ndarray:
    """build_dataset.py:68-88 (get_sample_data_ego_pose_P / get_calibration_P): the rotation matrix of the quaternion (w, x, y, z) and the
    translation, both rounded to float32, in a float64 4x4.  The quaternion is normalised first, as pyquaternion does (parity with
    pyquaternion itself is unpinned; tests hold this against scipy)."""
    q = np.asarray(rotation_wxyz, dtype=np.float64)
    w, x, y, z = q / np.linalg.norm(q)
    R = np.array([[1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - z * w), 2.0 * (x * z + y * w)],
                  [2.0 * (x * y + z * w), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - x * w)],
                  [2.0 * (x * z - y * w), 2.0 * (y * z + x * w), 1.0 - 2.0 * (x * x + y * y)]])
    P = np.identity(4)
    P[0:3, 0:3] = R.astype(np.float32)
    P[0:3, 3] = np.asarray(translation, dtype=np.float64).astype(np.float32)
    return P


def sweep_transforms(P_oi: np.ndarray, P_oj_list: Sequence[np.ndarray], P_vehicle_lidar: np.ndarray) -> np.ndarray:
    """build_dataset.py:142-143, 164-167: lidar frame of sweep j -> lidar frame of the key sweep, float64.  P_oi: ego pose of the key sweep,
    P_oj_list: ego poses of the other sweeps in accumulation order, P_vehicle_lidar: the lidar's calibration.  Returns (1 + len, 4, 4);
    entry 0, the key sweep's own, is the identity (and is never read)."""
    P_io = np.linalg.inv(np.asarray(P_oi, dtype=np.float64))
    P_vl = np.asarray(P_vehicle_lidar, dtype=np.float64)
    P_lv = np.linalg.inv(P_vl)
    out = [np.identity(4)]
    for P_oj in P_oj_list:
        P_ij = np.dot(P_io, np.asarray(P_oj, dtype=np.float64))
        out.append(np.dot(np.dot(P_lv, P_ij), P_vl))
    return np.stack(out, 0)


def camera_from_lidar(lidar_pose, lidar_calib, cam_pose, cam_calib) -> np.ndarray:
    """build_dataset.py:265-268: P_cam_pc, key sweep's lidar frame -> camera frame, float64"""
    return np.dot(np.linalg.inv(cam_calib), np.dot(np.linalg.inv(cam_pose), np.dot(lidar_pose, lidar_calib)))


def scaled_intrinsics(K, top: int = TOP_ROWS, scale: float = IMG_SCALE) -> np.ndarray:
    """build_dataset.py:254, 260: camera_matrix_cropping(K, 0, top), then camera_matrix_scaling(., scale), in float32"""
    Kc = np.array(K, dtype=np.float32)
    Kc[1, 2] -= np.float32(top)
    Ks = np.float32(scale) * Kc
    Ks[2, 2] = 1
    return Ks


def resized_hw(img_hw, top: int = TOP_ROWS, scale: float = IMG_SCALE):
    """build_dataset.py:256-258: size of the cropped and scaled image, Python round -> (h, w)"""
    return int(round((img_hw[0] - top) * scale)), int(round(img_hw[1] * scale))


# ---------------------------------------------------------------------------------------------- device side
def _p(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(a, dtype, device):
    """numpy array or tensor -> contiguous device tensor of `dtype`"""
    if isinstance(a, np.ndarray):
        a = torch.from_numpy(np.ascontiguousarray(a, dtype={torch.float32: np.float32, torch.float64: np.float64, torch.uint8: np.uint8}[dtype]))
    if a.dtype != dtype:
        raise _lib.CofiError("sweeps: expected a %s tensor, got %s" % (dtype, a.dtype))
    return a.to(device, non_blocking=True).contiguous()


class SweepBuilder:
    """The device buffers of the raw-sweep path, cached per size like FramePreparer's: the accumulated cloud, the voxel rows and the
    kernels' scratch (ops.Workspace) are reused by the next call, which overwrites what the previous one returned from `accumulate`
    and `voxel_downsample`; `to_camera` and `resize_u8` return fresh tensors.  One builder per stream."""

    def __init__(self, device="cuda"):
        self.device = torch.device(device)
        self._ws = ops.Workspace()
        self._pts = self._inten = self._vox = None
        self._cnt = None          # device counters: [accumulated, voxels, overflow, inside]
        self._host = None         # their pinned copy
        self.last: Dict = {}

    def _counters(self):
        if self._cnt is None:
            self._cnt = torch.zeros(4, dtype=torch.int32, device=self.device)
            self._host = torch.zeros(4, dtype=torch.int32, pin_memory=True)
        return self._cnt

    def _read(self, lo: int, hi: int):
        """one pinned copy + event wait on counters [lo, hi)"""
        self._host[lo:hi].copy_(self._cnt[lo:hi], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        ev.synchronize()
        return [int(v) for v in self._host[lo:hi]]

    # ---- accumulation
    def _accumulate(self, sweeps, transforms):
        """enqueue cofi_accumulate_sweeps -> (points buffer, intensity buffer, total rows); the kept count lands in counter 0"""
        lib = _lib.load()
        S = len(sweeps)
        if S < 1 or S > MAX_SWEEPS:
            raise _lib.CofiError("sweeps: between 1 and %d sweeps per sample" % MAX_SWEEPS)
        ld = int(sweeps[0].shape[-1])
        for s in sweeps:
            if s.ndim != 2 or s.shape[1] != ld or ld not in (4, 5):
                raise _lib.CofiError("sweeps: every sweep is (n, 5) or (n, 4) float32 rows [x y z intensity (ring)], all of one width")
        T = np.ascontiguousarray(transforms, dtype=np.float64) if not torch.is_tensor(transforms) else transforms
        if tuple(T.shape) != (S, 4, 4):
            raise _lib.CofiError("sweeps: transforms must be (%d, 4, 4) float64" % S)
        lens = [int(s.shape[0]) for s in sweeps]
        total = sum(lens)
        cnt = self._counters()
        if self._pts is None or self._pts.shape[0] < max(total, 1):
            self._pts = torch.empty((max(total, 1), 3), dtype=torch.float64, device=self.device)
            self._inten = torch.empty((max(total, 1),), dtype=torch.float32, device=self.device)
        if total == 0:
            cnt[0:1].zero_()
            return self._pts, self._inten, 0
        if all(isinstance(s, np.ndarray) for s in sweeps):
            rows = _dev(np.concatenate([np.asarray(s, dtype=np.float32) for s in sweeps], 0), torch.float32, self.device)
        else:
            rows = torch.cat([_dev(s, torch.float32, self.device) for s in sweeps], 0).contiguous()
        offs = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)).to(self.device, non_blocking=True)
        Td = _dev(T, torch.float64, self.device)
        ws = self._ws.get(lib.cofi_accumulate_sweeps_workspace(total), self.device)
        _lib.check(lib.cofi_accumulate_sweeps(_p(rows), ld, _p(offs), S, total, _p(Td), _p(self._pts), _p(self._inten), _p(cnt), _p(ws), ws.numel(),
                                              _stream()), "cofi_accumulate_sweeps")
        return self._pts, self._inten, total

    def accumulate(self, sweeps, transforms):
        """sweeps: list of (n_j, 5) or (n_j, 4) float32 arrays / device tensors, the key sweep first; transforms (S, 4, 4) float64
        (sweep_transforms).  -> (points (n, 3) float64, intensity (n,) float32, n): the points outside the ego box, in the key sweep's
        lidar frame, in sweep order then original order.  Waits on the count."""
        pts, inten, _ = self._accumulate(sweeps, transforms)
        n = self._read(0, 1)[0]
        return pts[:n], inten[:n], n

    # ---- voxel grid
    def _voxel(self, points: torch.Tensor, intensity: torch.Tensor, voxel: float, cap: Optional[int]):
        lib = _lib.load()
        N = int(points.shape[0])
        if points.dim() != 2 or points.shape[1] != 3 or intensity.dim() != 1 or intensity.shape[0] != N or N < 1:
            raise _lib.CofiError("sweeps: the voxel grid takes (N, 3) float64 points and (N,) float32 intensities, N >= 1")
        cap = N if cap is None else int(cap)
        if self._vox is None or self._vox.shape[0] < cap:
            self._vox = torch.empty((cap, 4), dtype=torch.float32, device=self.device)
        cnt = self._counters()
        ws = self._ws.get(lib.cofi_voxel_downsample_f64_workspace(N), self.device)
        _lib.check(lib.cofi_voxel_downsample_f64(_p(points), _p(intensity), N, float(voxel), _p(self._vox), cap, _p(cnt[1:3]), _p(ws), ws.numel(),
                                                 _stream()), "cofi_voxel_downsample_f64")
        return self._vox, cap

    def _voxel_count(self, cap: int) -> int:
        n, overflow = self._read(1, 3)
        if overflow:
            raise _lib.CofiError("sweeps: the accumulated cloud spans more than 8192 voxels along an axis")
        return n

    def voxel_downsample(self, points, intensity, voxel: float = VOXEL_SIZE, cap: Optional[int] = None):
        """(N, 3) float64 points + (N,) float32 reflectance -> ((min(count, cap), 4) float32 rows [mean xyz | mean reflectance], count) in
        ascending voxel-index order.  The voxel index is taken from the float64 point.  Waits on the count; raises CofiError when the
        cloud spans more than 8192 voxels along an axis."""
        vox, cap = self._voxel(_dev(points, torch.float64, self.device), _dev(intensity, torch.float32, self.device), voxel, cap)
        n = self._voxel_count(cap)
        return vox[:min(n, cap)], n

    # ---- camera frame
    def _camera(self, rows: torch.Tensor, P, K, hw):
        lib = _lib.load()
        M = int(rows.shape[0])
        if rows.dim() != 2 or rows.shape[1] != 4 or M < 1:
            raise _lib.CofiError("sweeps: to_camera takes (M, 4) float32 rows, M >= 1")
        Pd = _dev(np.asarray(P, dtype=np.float64) if not torch.is_tensor(P) else P, torch.float64, self.device)
        Kd = _dev(np.asarray(K, dtype=np.float32) if not torch.is_tensor(K) else K, torch.float32, self.device)
        if tuple(Pd.shape) != (4, 4) or tuple(Kd.shape) != (3, 3):
            raise _lib.CofiError("sweeps: P is a float64 4x4, K a float32 3x3")
        out = torch.empty((4, M), dtype=torch.float32, device=self.device)
        cnt = self._counters()
        _lib.check(lib.cofi_sweeps_to_camera(_p(rows), M, _p(Pd), _p(Kd), int(hw[0]), int(hw[1]), _p(out), _p(cnt[3:4]), _stream()),
                   "cofi_sweeps_to_camera")
        return out

    def to_camera(self, rows, P, K, hw):
        """(M, 4) float32 voxel rows, P_cam_pc (float64 4x4), K of the scaled image (float32 3x3), hw = its (h, w) -> ((4, M) float32 cloud
        [camera-frame xyz | reflectance], number of points that project into the picture).  Waits on the count."""
        out = self._camera(_dev(rows, torch.float32, self.device), P, K, hw)
        return out, self._read(3, 4)[0]

    # ---- image
    def resize_u8(self, img, top: int = TOP_ROWS, scale: float = IMG_SCALE) -> torch.Tensor:
        """(H, W, 3) uint8 -> the top `top` rows dropped, cv2.resize(INTER_LINEAR) by `scale` -> (h, w, 3) uint8 on the device (no wait)"""
        lib = _lib.load()
        img = _dev(img, torch.uint8, self.device)
        if img.dim() != 3 or img.shape[2] != 3 or not 0 <= top < img.shape[0]:
            raise _lib.CofiError("sweeps: the image must be (H, W, 3) uint8 with more than `top` rows")
        h, w = resized_hw(img.shape[:2], top, scale)
        if h < 1 or w < 1:
            raise _lib.CofiError("sweeps: the scaled image is empty")
        out = torch.empty((h, w, 3), dtype=torch.uint8, device=self.device)
        _lib.check(lib.cofi_resize_image_u8(_p(img), img.shape[0], img.shape[1], int(top), h, w, _p(out), _stream()), "cofi_resize_image_u8")
        return out

    # ---- one sample
    def build_sample(self, sweeps, transforms, cameras, opt=None, min_points: int = MIN_POINTS, min_inside: int = MIN_INSIDE,
                     voxel: float = VOXEL_SIZE) -> Optional[Dict]:
        """make_dataset (build_dataset.py:217-300) for one sample.  cameras: list of (img (H, W, 3) uint8, K (3, 3), P_cam_pc (4, 4) float64)
        candidates, tried in order; opt: crop_original_top_rows / img_scale are read from it when present (data/options.py:71-72).
        Returns {"pc": (4, M) float32 device, "img": (h, w, 3) uint8 device, "K": float32 (3, 3), "P": float64 (4, 4), "inside",
        "accumulated", "voxels", "camera"} or None when the sample is rejected; `last` then holds {"rejected": "accumulated" | "voxels" |
        "inside", ...counts so far}.  The image is resized for the accepted candidate only."""
        top = int(getattr(opt, "crop_original_top_rows", TOP_ROWS))
        scale = float(getattr(opt, "img_scale", IMG_SCALE))
        self.last = {}
        pts, inten, _ = self._accumulate(sweeps, transforms)
        n = self._read(0, 1)[0]
        self.last["accumulated"] = n
        if n < min_points:
            self.last["rejected"] = "accumulated"
            return None
        vox, cap = self._voxel(pts[:n], inten[:n], voxel, None)
        m = self._voxel_count(cap)
        self.last["voxels"] = m
        if m < min_points:
            self.last["rejected"] = "voxels"
            return None
        self.last["inside"] = []
        for ci, (img, K, P) in enumerate(cameras):
            Ks = scaled_intrinsics(K, top, scale)
            pc = self._camera(vox[:m], P, Ks, resized_hw(img.shape[:2], top, scale))
            inside = self._read(3, 4)[0]
            self.last["inside"].append(inside)
            if inside > min_inside:
                return {"pc": pc, "img": self.resize_u8(img, top, scale), "K": Ks, "P": np.array(P, dtype=np.float64), "inside": inside,
                        "accumulated": n, "voxels": m, "camera": ci}
        self.last["rejected"] = "inside"
        return None


_builders: Dict = {}


def _builder(device="cuda") -> SweepBuilder:
    dev = torch.device(device)
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    key = (dev, _stream())
    if key not in _builders:
        _builders[key] = SweepBuilder(dev)
    return _builders[key]


def accumulate(sweeps, transforms, device="cuda"):
    """SweepBuilder.accumulate on the module's builder of this device and stream"""
    return _builder(device).accumulate(sweeps, transforms)


def voxel_downsample(points, intensity, voxel: float = VOXEL_SIZE, cap: Optional[int] = None, device="cuda"):
    """SweepBuilder.voxel_downsample on the module's builder of this device and stream"""
    return _builder(device).voxel_downsample(points, intensity, voxel, cap)


def to_camera(rows, P, K, hw, device="cuda"):
    """SweepBuilder.to_camera on the module's builder of this device and stream"""
    return _builder(device).to_camera(rows, P, K, hw)


def resize_u8(img, top: int = TOP_ROWS, scale: float = IMG_SCALE, device="cuda"):
    """SweepBuilder.resize_u8 on the module's builder of this device and stream"""
    return _builder(device).resize_u8(img, top, scale)


def build_sample(sweeps, transforms, cameras, opt=None, min_points: int = MIN_POINTS, min_inside: int = MIN_INSIDE, voxel: float = VOXEL_SIZE,
                 device="cuda"):
    """SweepBuilder.build_sample on the module's builder of this device and stream; `build_sample.last` holds the counts and, after a
    rejection (None), the reason."""
    b = _builder(device)
    out = b.build_sample(sweeps, transforms, cameras, opt, min_points, min_inside, voxel)
    build_sample.last = b.last
    return out


build_sample.last = {}
