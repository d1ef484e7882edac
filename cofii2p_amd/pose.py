"""Camera pose from the fine matches + the registration errors the reference's evaluation reports
(evaluation/eval_all.py:16-22, 107-117) — row f1 of SURVEY.md §8.

    ok, R, t, inliers = solve_pnp_ransac(coarse_pc_points, fine_xy.T, K)          # cv2.solvePnPRansac(..., iterationsCount=10000)
    rte, rre = get_P_diff(T_pred, P_gt)                                            # eval_all.py:16-22

`solve_pnp_ransac` runs on the device (cofi_pnp_ransac: P3P hypotheses in parallel, consensus by reprojection error, LM refit);
its arguments are CUDA tensors and nothing is copied to the host unless the caller asks for `ok`.  OpenCV is not available in
this environment, so equality with cv2's result is not pinned; the implementation is checked against
oracle/pnp_oracle.py and against ground-truth poses of synthetic correspondences.

For the B frames of a stack-mode submission: `solve_pnp_ransac_batch` (cofi_pnp_ransac_batch: all frames in two launches, operands and
intrinsics read on the device in the layout the forward leaves them, frame f bit-identical to the per-frame call with seed + f) and
`pose_errors` (cofi_pose_errors: get_P_diff of B poses on the device).

For the S rigs of a rig submission whose C cameras are bolted to one body: `solve_pnp_ransac_rig` (cofi_pnp_ransac_rig: ONE pose per
rig, rig <- cloud, from the matches of all its cameras; extrinsics camera <- rig through `rig_extrinsics`; per-image poses composed from
it)."""
from typing import Optional

import numpy as np
import torch

from . import _lib, ops


def solve_pnp_ransac(object_points: torch.Tensor, image_points: torch.Tensor, K, iterations: int = 10000, reproj_error: float = 8.0,
                     seed: int = 0, refine_iters: int = 20, count: Optional[torch.Tensor] = None):
    """object_points (n,3), image_points (n,2) float32 CUDA, K (3,3) (tensor / array: fx, fy, cx, cy are read on the host).
    count (optional int32 device tensor): number of valid rows, read on the device (capacity-sized inputs of the test-mode
    forward).  Returns (result, R (3,3), t (3,), inlier_mask (n,) uint8) as device tensors; result = int32 [success, inliers,
    winning hypothesis]."""
    lib = _lib.load()
    for t_, name, w in ((object_points, "object_points", 3), (image_points, "image_points", 2)):
        if not t_.is_cuda or t_.dtype != torch.float32 or t_.dim() != 2 or t_.shape[1] != w or not t_.is_contiguous():
            raise _lib.CofiError("solve_pnp_ransac: %s must be a contiguous CUDA float32 (n,%d) tensor" % (name, w))
    n = object_points.shape[0]
    if image_points.shape[0] != n or n == 0:
        raise _lib.CofiError("solve_pnp_ransac: need n >= 1 correspondences of equal count")
    Kh = K.detach().cpu().numpy() if torch.is_tensor(K) else np.asarray(K)
    dev = object_points.device
    ws = torch.empty(lib.cofi_pnp_ransac_workspace(iterations), dtype=torch.uint8, device=dev)
    pose = torch.empty(12, dtype=torch.float32, device=dev)
    result = torch.empty(3, dtype=torch.int32, device=dev)
    mask = torch.empty(n, dtype=torch.uint8, device=dev)
    rc = lib.cofi_pnp_ransac(ops._p(object_points), ops._p(image_points), ops._p(count), n, float(Kh[0, 0]), float(Kh[1, 1]),
                             float(Kh[0, 2]), float(Kh[1, 2]), int(iterations), float(reproj_error), int(seed) & 0xFFFFFFFF,
                             int(refine_iters), ops._p(ws), ws.numel(), ops._p(pose), ops._p(result), ops._p(mask), ops._stream())
    _lib.check(rc, "cofi_pnp_ransac")
    return result, pose[:9].view(3, 3), pose[9:], mask


def _batch_operands(object_points, image_points, K, count, coord_major, what):
    """checks of the batched call -> (B, cap, K on the device, count pointer, count stride)"""
    E = _lib.CofiError
    if not (torch.is_tensor(object_points) and object_points.is_cuda and object_points.dtype == torch.float32 and object_points.dim() == 3
            and object_points.shape[2] == 3 and object_points.is_contiguous()):
        raise E("%s: object_points must be a contiguous CUDA float32 (B,cap,3) tensor" % what)
    B, cap = object_points.shape[0], object_points.shape[1]
    want = (B, 2, cap) if coord_major else (B, cap, 2)
    if not (torch.is_tensor(image_points) and image_points.is_cuda and image_points.dtype == torch.float32 and tuple(image_points.shape) == want
            and image_points.is_contiguous()):
        raise E("%s: image_points must be a contiguous CUDA float32 %s tensor (coord_major=%s)" % (what, want, bool(coord_major)))
    if B == 0 or cap == 0:
        raise E("%s: need B >= 1 frames of capacity >= 1" % what)
    dev = object_points.device
    if not torch.is_tensor(K):
        K = torch.as_tensor(np.asarray(K, dtype=np.float32))
    if tuple(K.shape) != (B, 3, 3):
        raise E("%s: K must be (B,3,3) = %s, got %s" % (what, (B, 3, 3), tuple(K.shape)))
    if K.is_cuda:   # read in place by the kernels: never copied to the host
        if K.dtype != torch.float32 or not K.is_contiguous() or K.device != dev:
            raise E("%s: a device K must be a contiguous float32 tensor on the device of the points" % what)
    else:
        K = K.to(torch.float32).contiguous().to(dev, non_blocking=True)
    cstride = 0
    if count is not None:
        if not (torch.is_tensor(count) and count.is_cuda and count.dtype == torch.int32 and count.dim() == 1 and count.shape[0] == B
                and (B == 1 or count.stride(0) >= 1)):
            raise E("%s: count must be an int32 CUDA tensor of B elements (a strided 1-D view is read in place)" % what)
        cstride = max(1, count.stride(0))
    return B, cap, K, count, cstride


def pnp_batch_workspace(iterations: int, frames: int) -> int:
    return _lib.load().cofi_pnp_ransac_batch_workspace(int(iterations), int(frames))


def pnp_batch_workspace_views(ws: torch.Tensor, iterations: int, frames: int):
    """(keys, poses): views of a workspace of solve_pnp_ransac_batch_into in the layout cofi_pnp_ransac_batch documents - one consensus
    key per frame (padded to 64 bytes), then one slab of iterations x 12 floats per frame.  keys (frames,) int64, decoded by
    pnp_decode_key; poses (frames, iterations, 12) float32: row h of a frame is hypothesis h (R row-major | t), written only if that
    hypothesis produced a pose.  For tests and tools: the product never looks inside the workspace."""
    iterations, frames = int(iterations), int(frames)
    need = pnp_batch_workspace(iterations, frames)
    slab_bytes = frames * iterations * 12 * 4
    if not (torch.is_tensor(ws) and ws.dtype == torch.uint8 and ws.dim() == 1 and ws.is_contiguous() and need > 0 and ws.numel() >= need):
        raise _lib.CofiError("pnp_batch_workspace_views: ws must be a contiguous uint8 tensor of at least pnp_batch_workspace(%d, %d) = %d bytes"
                             % (iterations, frames, need))
    key_bytes = need - slab_bytes   # the padded key block: the size is the library's own
    return ws[:8 * frames].view(torch.int64), ws[key_bytes:need].view(torch.float32).view(frames, iterations, 12)


def pnp_decode_key(key):
    """(inliers, hypothesis) of a consensus key (inliers << 32 | 0xFFFFFFFF - hypothesis: most inliers win, lowest id on ties).
    A key of 0 - no hypothesis of the frame produced a pose - decodes to (0, 0xFFFFFFFF)."""
    key = int(key)
    return key >> 32, 0xFFFFFFFF - (key & 0xFFFFFFFF)


def solve_pnp_ransac_batch_into(object_points, image_points, K, count, ws, pose, result, mask, iterations: int = 10000,
                                reproj_error: float = 8.0, seed: int = 0, refine_iters: int = 20, coord_major: bool = False):
    """solve_pnp_ransac_batch into caller-owned buffers (ws uint8, pose (B,12) float32, result (B,3) int32, mask (B,cap) uint8): the
    form a pipeline with static buffers uses.  Enqueues a memset and two kernels on the current stream; nothing else."""
    lib = _lib.load()
    B, cap, K, count, cstride = _batch_operands(object_points, image_points, K, count, coord_major, "solve_pnp_ransac_batch")
    for t_, shape, dt in ((pose, (B, 12), torch.float32), (result, (B, 3), torch.int32), (mask, (B, cap), torch.uint8)):
        if not (t_.is_cuda and t_.dtype == dt and tuple(t_.shape) == shape and t_.is_contiguous()):
            raise _lib.CofiError("solve_pnp_ransac_batch: output buffers must be contiguous CUDA tensors pose (B,12) float32, result (B,3) int32, mask (B,cap) uint8")
    rc = lib.cofi_pnp_ransac_batch(ops._p(object_points), 3 * cap, ops._p(image_points), 2 * cap, 1 if coord_major else 0, ops._p(count), cstride,
                                   ops._p(K), cap, B, int(iterations), float(reproj_error), int(seed) & 0xFFFFFFFF, int(refine_iters),
                                   ops._p(ws), ws.numel(), ops._p(pose), ops._p(result), ops._p(mask), ops._stream())
    _lib.check(rc, "cofi_pnp_ransac_batch")
    return result, pose[:, :9].view(B, 3, 3), pose[:, 9:], mask


def solve_pnp_ransac_batch(object_points: torch.Tensor, image_points: torch.Tensor, K, count: Optional[torch.Tensor] = None,
                           iterations: int = 10000, reproj_error: float = 8.0, seed: int = 0, refine_iters: int = 20,
                           coord_major: bool = False):
    """The pose of every frame of a stack-mode submission in one pass (cofi_pnp_ransac_batch): frame f is bit-identical to
    solve_pnp_ransac(object_points[f, :n_f], image_points[f, :n_f], K[f], seed=seed + f).

    object_points (B,cap,3); image_points (B,cap,2), or (B,2,cap) with coord_major=True (the `fine_xy` the forward writes: no
    transpose); K (B,3,3): a float32 device tensor is read by the kernels in place, a host tensor / array is uploaded - the intrinsics
    never travel to the host; count: int32 device tensor of B valid-row counts, possibly a strided view such as count_all[:, 0]
    (None: every row of every frame is valid).  Returns (result (B,3) int32 [success, inliers, winning hypothesis], R (B,3,3), t (B,3),
    inlier_mask (B,cap) uint8) as device tensors.  No host synchronisation: the call can be captured in a hipGraph."""
    B, cap, K, count, _ = _batch_operands(object_points, image_points, K, count, coord_major, "solve_pnp_ransac_batch")
    dev = object_points.device
    ws = torch.empty(pnp_batch_workspace(iterations, B), dtype=torch.uint8, device=dev)
    pose = torch.empty((B, 12), dtype=torch.float32, device=dev)
    result = torch.empty((B, 3), dtype=torch.int32, device=dev)
    mask = torch.empty((B, cap), dtype=torch.uint8, device=dev)
    return solve_pnp_ransac_batch_into(object_points, image_points, K, count, ws, pose, result, mask, iterations, reproj_error, seed,
                                       refine_iters, coord_major)


def rig_extrinsics(E, cameras: int, device):
    """The extrinsics of a rig of C = `cameras` cameras as the rig solver reads them -> (ext, rig_stride): a contiguous float32 device
    tensor of 12-float rows [R row-major | t], (C,12) with rig_stride 0 (one set shared by all rigs) or (S,C,12) with rig_stride 12 C (one
    set per rig).  Convention: camera <- rig, Y_cam = R_c Y_rig + t_c.  E: (C,4,4), (C,3,4), (S,C,4,4) or (S,C,3,4).  A host array /
    tensor is checked (rotation block orthonormal to within 1e-4, the rounding of a calibration file; bottom row [0,0,0,1]) and
    uploaded; a device tensor is read as it is, without a download."""
    Err = _lib.CofiError
    C = int(cameras)
    shape = tuple(E.shape) if hasattr(E, "shape") else tuple(np.asarray(E).shape)
    if C < 1 or len(shape) not in (3, 4) or shape[-1] != 4 or shape[-2] not in (3, 4) or shape[-3] != C or (len(shape) == 4 and shape[0] < 1):
        raise Err("rig_extrinsics: need (C,4,4), (C,3,4), (S,C,4,4) or (S,C,3,4) with C = %d cameras, got %s" % (C, shape))
    if torch.is_tensor(E) and E.is_cuda:
        ext = E[..., :3, :]
    else:
        Eh = E.detach().cpu().numpy() if torch.is_tensor(E) else np.asarray(E)
        Eh = Eh.astype(np.float64)
        if not np.isfinite(Eh).all():
            raise Err("rig_extrinsics: non-finite entries")
        if shape[-2] == 4 and not np.array_equal(Eh[..., 3, :], np.broadcast_to(np.array([0.0, 0.0, 0.0, 1.0]), Eh[..., 3, :].shape)):
            raise Err("rig_extrinsics: the bottom row of every matrix must be [0, 0, 0, 1]")
        R = Eh[..., :3, :3]
        off = np.abs(R @ np.swapaxes(R, -1, -2) - np.eye(3)).max()
        if off > 1e-4 or (np.linalg.det(R) < 0).any():
            raise Err("rig_extrinsics: a rotation block is not orthonormal to within 1e-4 (max |R R^T - I| = %.3g) or is a reflection" % off)
        ext = torch.from_numpy(np.ascontiguousarray(Eh[..., :3, :], dtype=np.float32))
    # [R | t] rows (3,4) -> R row-major (9) | t (3)
    ext = torch.cat([ext[..., :3].reshape(shape[:-2] + (9,)), ext[..., 3]], -1).to(device=device, dtype=torch.float32).contiguous()
    return ext, (12 * C if ext.dim() == 3 else 0)


def pnp_rig_workspace(iterations: int, rigs: int) -> int:
    return _lib.load().cofi_pnp_ransac_rig_workspace(int(iterations), int(rigs))


def pnp_rig_workspace_views(ws: torch.Tensor, iterations: int, rigs: int):
    """(keys, poses): views of a workspace of solve_pnp_ransac_rig_into, as pnp_batch_workspace_views with one key and one slab per RIG:
    keys (rigs,) int64, poses (rigs, iterations, 12) float32 - row h of a rig is hypothesis h as a RIG pose (rig <- cloud), written only
    if that hypothesis produced a pose.  For tests and tools."""
    iterations, rigs = int(iterations), int(rigs)
    need = pnp_rig_workspace(iterations, rigs)
    slab_bytes = rigs * iterations * 12 * 4
    if not (torch.is_tensor(ws) and ws.dtype == torch.uint8 and ws.dim() == 1 and ws.is_contiguous() and need > 0 and ws.numel() >= need):
        raise _lib.CofiError("pnp_rig_workspace_views: ws must be a contiguous uint8 tensor of at least pnp_rig_workspace(%d, %d) = %d bytes"
                             % (iterations, rigs, need))
    key_bytes = need - slab_bytes
    return ws[:8 * rigs].view(torch.int64), ws[key_bytes:need].view(torch.float32).view(rigs, iterations, 12)


def _rig_operands(object_points, image_points, K, extrinsics, cameras, count, coord_major, what):
    """checks of the rig call -> (B, cap, S, K, count, count stride, ext, ext rig stride)"""
    B, cap, K, count, cstride = _batch_operands(object_points, image_points, K, count, coord_major, what)
    if not isinstance(cameras, int) or cameras < 1:
        raise _lib.CofiError("%s: cameras must be an integer >= 1, got %r" % (what, cameras))
    if B % cameras:
        raise _lib.CofiError("%s: B = %d images are no whole number of rigs of C = %d cameras" % (what, B, cameras))
    S = B // cameras
    if isinstance(extrinsics, tuple):   # (ext, rig_stride) of rig_extrinsics
        ext, estride = extrinsics
        if not (torch.is_tensor(ext) and ext.is_cuda and ext.device == object_points.device and ext.dtype == torch.float32 and ext.is_contiguous()
                and tuple(ext.shape) in ((cameras, 12), (S, cameras, 12)) and estride == (12 * cameras if ext.dim() == 3 else 0)):
            raise _lib.CofiError("%s: extrinsics given as (ext, rig_stride) must be what rig_extrinsics returns for C = %d cameras%s"
                                 % (what, cameras, " and S = %d rigs" % S))
    else:
        ext, estride = rig_extrinsics(extrinsics, cameras, object_points.device)
        if ext.dim() == 3 and ext.shape[0] != S:
            raise _lib.CofiError("%s: per-rig extrinsics for %d rigs, but B / C = %d" % (what, ext.shape[0], S))
    return B, cap, S, K, count, cstride, ext, estride


def solve_pnp_ransac_rig_into(object_points, image_points, K, extrinsics, cameras, count, ws, rig_pose, rig_result, pose, result, mask,
                              iterations: int = 10000, reproj_error: float = 8.0, seed: int = 0, refine_iters: int = 20,
                              coord_major: bool = False):
    """solve_pnp_ransac_rig into caller-owned buffers (ws uint8, rig_pose (S,12) float32, rig_result (S,3) int32, pose (B,12) float32,
    result (B,3) int32, mask (B,cap) uint8).  extrinsics: what solve_pnp_ransac_rig takes, or the pair rig_extrinsics returned (nothing
    is converted then).  Enqueues a memset and two kernels on the current stream; nothing else."""
    lib = _lib.load()
    what = "solve_pnp_ransac_rig"
    B, cap, S, K, count, cstride, ext, estride = _rig_operands(object_points, image_points, K, extrinsics, cameras, count, coord_major, what)
    for t_, shape, dt in ((rig_pose, (S, 12), torch.float32), (rig_result, (S, 3), torch.int32), (pose, (B, 12), torch.float32),
                          (result, (B, 3), torch.int32), (mask, (B, cap), torch.uint8)):
        if not (torch.is_tensor(t_) and t_.is_cuda and t_.dtype == dt and tuple(t_.shape) == shape and t_.is_contiguous()):
            raise _lib.CofiError("%s: output buffers must be contiguous CUDA tensors rig_pose (S,12) float32, rig_result (S,3) int32, pose (B,12) "
                                 "float32, result (B,3) int32, mask (B,cap) uint8" % what)
    if not (torch.is_tensor(ws) and ws.is_cuda and ws.dtype == torch.uint8 and ws.is_contiguous()):
        raise _lib.CofiError("%s: ws must be a contiguous CUDA uint8 tensor" % what)
    rc = lib.cofi_pnp_ransac_rig(ops._p(object_points), 3 * cap, ops._p(image_points), 2 * cap, 1 if coord_major else 0, ops._p(count), cstride,
                                 ops._p(K), ops._p(ext), int(estride), cap, int(cameras), S, int(iterations), float(reproj_error),
                                 int(seed) & 0xFFFFFFFF, int(refine_iters), ops._p(ws), ws.numel(), ops._p(rig_pose), ops._p(rig_result),
                                 ops._p(pose), ops._p(result), ops._p(mask), ops._stream())
    _lib.check(rc, "cofi_pnp_ransac_rig")
    return ({"result": rig_result, "R": rig_pose[:, :9].view(S, 3, 3), "t": rig_pose[:, 9:]},
            {"result": result, "R": pose[:, :9].view(B, 3, 3), "t": pose[:, 9:], "inliers": mask})


def solve_pnp_ransac_rig(object_points: torch.Tensor, image_points: torch.Tensor, K, extrinsics, cameras: int,
                         count: Optional[torch.Tensor] = None, iterations: int = 10000, reproj_error: float = 8.0, seed: int = 0,
                         refine_iters: int = 20, coord_major: bool = False):
    """ONE pose per rig from the matches of all its cameras (cofi_pnp_ransac_rig).  The operands are those of solve_pnp_ransac_batch for
    B = S * C images, image f = s * C + c being camera c of rig s (the layout of forward_async(..., cameras=C)); extrinsics: (C,4,4) /
    (C,3,4) shared by all rigs or (S,C,4,4) / (S,C,3,4), camera <- rig (Y_cam = R_c Y_rig + t_c), host array or device tensor (see
    rig_extrinsics).  Every hypothesis is a P3P solve in one camera - drawn in proportion to the cameras' rows among those with usable
    intrinsics and at least 4 rows - carried into the rig frame and scored over every camera; the winner is refitted on all cameras'
    inliers.  Cameras with fewer than 4 matches therefore contribute, but a rig whose cameras ALL have fewer than 4 fails even if the rows
    add up to more: there is no minimal solver across cameras (generalised P3P) here.  Rig s uses seed + s; at C = 1 with identity
    extrinsics the call is solve_pnp_ransac_batch.

    Returns (rig, per_image): rig = {"result" (S,3) int32 [success, inliers over all cameras, hypothesis], "R" (S,3,3), "t" (S,3)} is the
    pose rig <- cloud; per_image = {"result" (B,3) [rig success, this image's inliers, hypothesis], "R" (B,3,3), "t" (B,3), "inliers"
    (B,cap) uint8} holds E_c o rig pose, so whatever reads per-image poses keeps working.  A failed rig: [0,0,-1], identity poses, zero
    masks.  Device tensors, no host synchronisation: the call can be captured in a hipGraph."""
    B, cap, S, K, count, _, ext, estride = _rig_operands(object_points, image_points, K, extrinsics, cameras, count, coord_major,
                                                         "solve_pnp_ransac_rig")
    dev = object_points.device
    ws = torch.empty(pnp_rig_workspace(iterations, S), dtype=torch.uint8, device=dev)
    rig_pose = torch.empty((S, 12), dtype=torch.float32, device=dev)
    rig_result = torch.empty((S, 3), dtype=torch.int32, device=dev)
    pose = torch.empty((B, 12), dtype=torch.float32, device=dev)
    result = torch.empty((B, 3), dtype=torch.int32, device=dev)
    mask = torch.empty((B, cap), dtype=torch.uint8, device=dev)
    return solve_pnp_ransac_rig_into(object_points, image_points, K, (ext, estride), cameras, count, ws, rig_pose, rig_result, pose, result,
                                     mask, iterations, reproj_error, seed, refine_iters, coord_major)


def pose_errors(pose, P_gt) -> torch.Tensor:
    """[RTE, RRE] of B predicted poses against B ground-truth matrices on the device (cofi_pose_errors; get_P_diff per frame,
    evaluation/eval_all.py:16-22).  pose: a (B,12) float32 device tensor (R row-major | t) or a pair (R (B,3,3), t (B,3)); P_gt (B,4,4)
    float64 or float32 (a host tensor / array is uploaded).  Returns a (B,2) float64 device tensor; nothing is synchronised."""
    lib = _lib.load()
    if isinstance(pose, (tuple, list)):
        R, t = pose
        if not (torch.is_tensor(R) and torch.is_tensor(t) and R.dim() == 3 and tuple(R.shape[1:]) == (3, 3) and tuple(t.shape) == (R.shape[0], 3)):
            raise _lib.CofiError("pose_errors: (R, t) must be (B,3,3) and (B,3) tensors")
        pose = torch.cat([R.reshape(R.shape[0], 9), t], 1)
    if not (torch.is_tensor(pose) and pose.is_cuda and pose.dtype == torch.float32 and pose.dim() == 2 and pose.shape[1] == 12):
        raise _lib.CofiError("pose_errors: pose must be a CUDA float32 (B,12) tensor or a pair (R (B,3,3), t (B,3))")
    pose = pose.contiguous()
    B = pose.shape[0]
    if not torch.is_tensor(P_gt):
        P_gt = torch.as_tensor(np.asarray(P_gt))
    if tuple(P_gt.shape) != (B, 4, 4) or P_gt.dtype not in (torch.float64, torch.float32) or B == 0:
        raise _lib.CofiError("pose_errors: P_gt must be a (B,4,4) float64 or float32 tensor with B = %d >= 1" % B)
    P_gt = P_gt.to(pose.device, non_blocking=True).contiguous()
    out = torch.empty((B, 2), dtype=torch.float64, device=pose.device)
    _lib.check(lib.cofi_pose_errors(ops._p(pose), ops._p(P_gt), 1 if P_gt.dtype == torch.float64 else 0, B, ops._p(out), ops._stream()),
               "cofi_pose_errors")
    return out


# ---------------------------------------------------------------------------------------------------- pose uncertainty
# The 6 x 6 Gauss-Newton covariance of the refit's least-squares problem at the pose the solver returned, over the consensus set it wrote
# into the masks (cofi_pose_covariance*; DESIGN.md, "Pose uncertainty").  Tangent vector (omega, v), rotation first, of the left-multiplied
# perturbation R' = exp(omega) R, t' = exp(omega) t + v.  cov, info (.., 6, 6) float64, exactly symmetric; stat (.., 4) float64 =
# [ok, rows used, sigma_hat^2, min_pivot]; ok = 0 goes with all-zero matrices.  NOT a model of outliers inside the gate or of the choice of
# the consensus set.
def _sigma(sigma_px) -> float:
    """None / True: estimate the pixel variance (0 for the kernel); a number: the given 1-sigma pixel noise"""
    if sigma_px is None or sigma_px is True:
        return 0.0
    s = float(sigma_px)
    if not (s > 0.0 and np.isfinite(s)):
        raise _lib.CofiError("pose covariance: sigma_px must be a finite number > 0 (or None to estimate it), got %r" % (sigma_px,))
    return s


def _pose12(pose, frames, what):
    """(R (F,3,3), t (F,3)) or (F,12) -> a contiguous (F,12) float32 buffer; views of one buffer, as the solvers return them, are not copied"""
    if isinstance(pose, (tuple, list)):
        R, t = pose
        if not (torch.is_tensor(R) and torch.is_tensor(t) and tuple(R.shape) == (frames, 3, 3) and tuple(t.shape) == (frames, 3)):
            raise _lib.CofiError("%s: (R, t) must be (%d,3,3) and (%d,3) tensors" % (what, frames, frames))
        base = R._base if R._base is not None else None
        if (base is not None and base is t._base and tuple(base.shape) == (frames, 12) and base.is_contiguous() and R.data_ptr() == base.data_ptr()
                and t.data_ptr() == base.data_ptr() + 36):
            pose = base
        else:
            pose = torch.cat([R.reshape(frames, 9), t], 1)
    if not (torch.is_tensor(pose) and pose.is_cuda and pose.dtype == torch.float32 and tuple(pose.shape) == (frames, 12) and pose.is_contiguous()):
        raise _lib.CofiError("%s: pose must be a contiguous CUDA float32 (%d,12) tensor or a pair (R, t)" % (what, frames))
    return pose


def _cov_buffers(frames, cov, info, stat, dev, what):
    for t_, shape in ((cov, (frames, 6, 6)), (info, (frames, 6, 6)), (stat, (frames, 4))):
        if not (torch.is_tensor(t_) and t_.is_cuda and t_.device == dev and t_.dtype == torch.float64 and tuple(t_.shape) == shape
                and t_.is_contiguous()):
            raise _lib.CofiError("%s: output buffers must be contiguous CUDA float64 tensors cov (F,6,6), info (F,6,6), stat (F,4) with F = %d"
                                 % (what, frames))


def _solver_outputs(result, mask, frames, images, cap, dev, what):
    if not (torch.is_tensor(result) and result.is_cuda and result.device == dev and result.dtype == torch.int32
            and tuple(result.shape) == (frames, 3) and result.is_contiguous()):
        raise _lib.CofiError("%s: result must be the solver's contiguous CUDA int32 (%d,3) tensor" % (what, frames))
    if not (torch.is_tensor(mask) and mask.is_cuda and mask.device == dev and mask.dtype == torch.uint8 and tuple(mask.shape) == (images, cap)
            and mask.is_contiguous()):
        raise _lib.CofiError("%s: inlier_mask must be the solver's contiguous CUDA uint8 (%d,%d) tensor" % (what, images, cap))


def pose_covariance(object_points: torch.Tensor, image_points: torch.Tensor, K, pose, result: torch.Tensor, inlier_mask: torch.Tensor,
                    sigma_px=None, count: Optional[torch.Tensor] = None):
    """The covariance of ONE frame's pose (cofi_pose_covariance): the operands of solve_pnp_ransac, then what it returned - pose (12,) or
    (R, t), result (3,), inlier_mask (n,).  sigma_px: the 1-sigma pixel noise, None to estimate it from the residuals.
    Returns (cov (6,6), info (6,6), stat (4,)) float64 device tensors."""
    lib = _lib.load()
    what = "pose_covariance"
    for t_, name, w in ((object_points, "object_points", 3), (image_points, "image_points", 2)):
        if not (torch.is_tensor(t_) and t_.is_cuda and t_.dtype == torch.float32 and t_.dim() == 2 and t_.shape[1] == w and t_.is_contiguous()):
            raise _lib.CofiError("%s: %s must be a contiguous CUDA float32 (n,%d) tensor" % (what, name, w))
    n = object_points.shape[0]
    if image_points.shape[0] != n or n == 0:
        raise _lib.CofiError("%s: need n >= 1 correspondences of equal count" % what)
    dev = object_points.device
    if isinstance(pose, (tuple, list)):
        pose = (pose[0][None], pose[1][None])
    else:
        pose = pose.reshape(1, 12) if torch.is_tensor(pose) else pose
    pose = _pose12(pose, 1, what)
    _solver_outputs(result.reshape(1, 3) if torch.is_tensor(result) else result, inlier_mask[None] if torch.is_tensor(inlier_mask) else inlier_mask,
                    1, 1, n, dev, what)
    Kh = K.detach().cpu().numpy() if torch.is_tensor(K) else np.asarray(K)
    cov = torch.empty((6, 6), dtype=torch.float64, device=dev)
    info = torch.empty((6, 6), dtype=torch.float64, device=dev)
    stat = torch.empty(4, dtype=torch.float64, device=dev)
    rc = lib.cofi_pose_covariance(ops._p(object_points), ops._p(image_points), ops._p(count), n, float(Kh[0, 0]), float(Kh[1, 1]), float(Kh[0, 2]),
                                  float(Kh[1, 2]), ops._p(pose), ops._p(result), ops._p(inlier_mask), _sigma(sigma_px), ops._p(cov), ops._p(info),
                                  ops._p(stat), ops._stream())
    _lib.check(rc, "cofi_pose_covariance")
    return cov, info, stat


def pose_covariance_batch_into(object_points, image_points, K, count, pose, result, inlier_mask, cov, info, stat, sigma_px=None,
                               coord_major: bool = False):
    """pose_covariance_batch into caller-owned buffers (cov, info (B,6,6), stat (B,4) float64).  Enqueues one kernel on the current stream;
    nothing else."""
    lib = _lib.load()
    what = "pose_covariance_batch"
    B, cap, K, count, cstride = _batch_operands(object_points, image_points, K, count, coord_major, what)
    dev = object_points.device
    pose = _pose12(pose, B, what)
    _solver_outputs(result, inlier_mask, B, B, cap, dev, what)
    _cov_buffers(B, cov, info, stat, dev, what)
    rc = lib.cofi_pose_covariance_batch(ops._p(object_points), 3 * cap, ops._p(image_points), 2 * cap, 1 if coord_major else 0, ops._p(count),
                                        cstride, ops._p(K), cap, B, ops._p(pose), ops._p(result), ops._p(inlier_mask), _sigma(sigma_px),
                                        ops._p(cov), ops._p(info), ops._p(stat), ops._stream())
    _lib.check(rc, "cofi_pose_covariance_batch")
    return cov, info, stat


def pose_covariance_batch(object_points: torch.Tensor, image_points: torch.Tensor, K, pose, result: torch.Tensor, inlier_mask: torch.Tensor,
                          sigma_px=None, count: Optional[torch.Tensor] = None, coord_major: bool = False):
    """The covariance of every frame's pose in one launch (cofi_pose_covariance_batch): the operands of solve_pnp_ransac_batch, then what
    it returned - pose (B,12) or (R (B,3,3), t (B,3)), result (B,3), inlier_mask (B,cap).  Frame f is bit-identical to pose_covariance on
    its slice.  Returns (cov (B,6,6), info (B,6,6), stat (B,4)) float64 device tensors; no host synchronisation."""
    B, _, _, _, _ = _batch_operands(object_points, image_points, K, count, coord_major, "pose_covariance_batch")
    dev = object_points.device
    cov = torch.empty((B, 6, 6), dtype=torch.float64, device=dev)
    info = torch.empty((B, 6, 6), dtype=torch.float64, device=dev)
    stat = torch.empty((B, 4), dtype=torch.float64, device=dev)
    return pose_covariance_batch_into(object_points, image_points, K, count, pose, result, inlier_mask, cov, info, stat, sigma_px, coord_major)


def pose_covariance_rig_into(object_points, image_points, K, extrinsics, cameras, count, rig_pose, rig_result, inlier_mask, cov, info, stat,
                             sigma_px=None, coord_major: bool = False):
    """pose_covariance_rig into caller-owned buffers (cov, info (S,6,6), stat (S,4) float64).  extrinsics: what solve_pnp_ransac_rig takes,
    or the pair rig_extrinsics returned (nothing is converted then).  Enqueues one kernel on the current stream; nothing else."""
    lib = _lib.load()
    what = "pose_covariance_rig"
    B, cap, S, K, count, cstride, ext, estride = _rig_operands(object_points, image_points, K, extrinsics, cameras, count, coord_major, what)
    dev = object_points.device
    rig_pose = _pose12(rig_pose, S, what)
    _solver_outputs(rig_result, inlier_mask, S, B, cap, dev, what)
    _cov_buffers(S, cov, info, stat, dev, what)
    rc = lib.cofi_pose_covariance_rig(ops._p(object_points), 3 * cap, ops._p(image_points), 2 * cap, 1 if coord_major else 0, ops._p(count),
                                      cstride, ops._p(K), ops._p(ext), int(estride), cap, int(cameras), S, ops._p(rig_pose), ops._p(rig_result),
                                      ops._p(inlier_mask), _sigma(sigma_px), ops._p(cov), ops._p(info), ops._p(stat), ops._stream())
    _lib.check(rc, "cofi_pose_covariance_rig")
    return cov, info, stat


def pose_covariance_rig(object_points: torch.Tensor, image_points: torch.Tensor, K, extrinsics, cameras: int, rig_pose,
                        rig_result: torch.Tensor, inlier_mask: torch.Tensor, sigma_px=None, count: Optional[torch.Tensor] = None,
                        coord_major: bool = False):
    """ONE covariance per rig, in the rig's tangent space (cofi_pose_covariance_rig): the operands of solve_pnp_ransac_rig, then what it
    returned - the rig's pose (S,12) or (R, t) and result (S,3), and the per-image inlier masks (B,cap).  The covariance of camera c's own
    pose follows with transport_covariance(cov, E_c).  Returns (cov (S,6,6), info (S,6,6), stat (S,4)) float64 device tensors."""
    B, _, S, K, count, _, ext, estride = _rig_operands(object_points, image_points, K, extrinsics, cameras, count, coord_major,
                                                       "pose_covariance_rig")
    dev = object_points.device
    cov = torch.empty((S, 6, 6), dtype=torch.float64, device=dev)
    info = torch.empty((S, 6, 6), dtype=torch.float64, device=dev)
    stat = torch.empty((S, 4), dtype=torch.float64, device=dev)
    return pose_covariance_rig_into(object_points, image_points, K, (ext, estride), cameras, count, rig_pose, rig_result, inlier_mask, cov, info,
                                    stat, sigma_px, coord_major)


def image_points(outs) -> torch.Tensor:
    """The image points (B, 2, cap), coordinate-major, that every consumer of a forward_async submission's matches reads - `outs` is
    handle["out"]: the sub-pixel matches "sub_xy_all" where the submission has them (forward_async(subpixel=True)), else the
    reference's "fine_xy_all".  The one place that choice is made: the pose tail, the covariance and the evaluation monitors ask here."""
    o0 = outs[0]
    return o0["sub_xy_all"] if "sub_xy_all" in o0 else o0["fine_xy_all"]


class PoseTail:
    """The pose tail of one forward_async slot: the buffers the slot owns - per (B, cap, iterations): ws, pose, result, mask, K; the rig
    set and the covariance sets, each made when a submission first asks for it - and the launches that fill them."""

    def __init__(self):
        self.sets = {}

    def enqueue(self, outs, K, iterations, seed, cameras=1, rig_ext=None, pose_cov=None):
        """the batched pose tail of a submission (with rig_ext = (ext, rig stride): the rig solve; with pose_cov = (sigma_px or None,): the
        covariance launch behind it), on the current stream -> (handle["pose"], K on the device, handle["rig_pose"] or None)"""
        if "coarse_pts_all" not in outs[0]:
            raise _lib.CofiError("forward_async(pose_K=...): the batched pose tail reads the outputs of match_finish, which serves fine "
                                 "feature maps of at most 128 channels; this model's fine map is wider")
        cpts, fxy, count = outs[0]["coarse_pts_all"], image_points(outs), outs[0]["count_all"][:, 0]
        B, cap, dev = cpts.shape[0], cpts.shape[1], cpts.device
        if not torch.is_tensor(K):
            K = torch.as_tensor(np.asarray(K, dtype=np.float32))
        if tuple(K.shape) not in ((B, 3, 3), (3, 3)):
            raise _lib.CofiError("forward_async: pose_K must be (B,3,3) = %s or (3,3), got %s" % ((B, 3, 3), tuple(K.shape)))
        key = (B, cap, int(iterations))
        b = self.sets.get(key)
        if b is None:
            b = self.sets[key] = {"ws": torch.empty(pnp_batch_workspace(iterations, B), dtype=torch.uint8, device=dev),
                                  "pose": torch.empty((B, 12), dtype=torch.float32, device=dev),
                                  "result": torch.empty((B, 3), dtype=torch.int32, device=dev),
                                  "mask": torch.empty((B, cap), dtype=torch.uint8, device=dev),
                                  "K": torch.empty((B, 3, 3), dtype=torch.float32, device=dev)}
        if not (K.is_cuda and K.device == dev and K.dtype == torch.float32 and K.dim() == 3 and K.is_contiguous()):
            b["K"].copy_(K, non_blocking=True)   # broadcasts a (3,3); a device K of another dtype is converted on the device
            K = b["K"]

        def covariance(holder, frames, launch, *operands):
            """one covariance launch into the float64 set `holder` owns for `frames` bodies -> the three handle entries"""
            c = holder.get("cov")
            if c is None:
                c = holder["cov"] = [torch.empty((frames,) + s, dtype=torch.float64, device=dev) for s in ((6, 6), (6, 6), (4,))]
            launch(cpts, fxy, K, *operands, b["mask"], *c, sigma_px=pose_cov[0], coord_major=True)
            return dict(zip(("cov", "info", "cov_stat"), c))

        if rig_ext is None:
            res, R, t, mask = solve_pnp_ransac_batch_into(cpts, fxy, K, count, b["ws"], b["pose"], b["result"], b["mask"],
                                                          iterations=iterations, seed=seed, coord_major=True)
            pose = {"result": res, "R": R, "t": t, "inliers": mask}
            if pose_cov is not None:
                pose.update(covariance(b, B, pose_covariance_batch_into, count, b["pose"], b["result"]))
            return pose, K, None
        S = B // cameras
        ext, estride = rig_ext
        r = b.get("rig")
        if r is None:
            r = b["rig"] = {"ws": torch.empty(pnp_rig_workspace(iterations, S), dtype=torch.uint8, device=dev),
                            "pose": torch.empty((S, 12), dtype=torch.float32, device=dev),
                            "result": torch.empty((S, 3), dtype=torch.int32, device=dev)}
        if not (ext.is_cuda and ext.device == dev):   # a host set: into a buffer of the slot, as K
            buf = r.get("ext")
            if buf is None or buf.shape != ext.shape:
                buf = r["ext"] = torch.empty(tuple(ext.shape), dtype=torch.float32, device=dev)
            buf.copy_(ext, non_blocking=True)
            ext = buf
        rig, per = solve_pnp_ransac_rig_into(cpts, fxy, K, (ext, estride), cameras, count, r["ws"], r["pose"], r["result"],
                                             b["pose"], b["result"], b["mask"], iterations=iterations, seed=seed, coord_major=True)
        if pose_cov is not None:
            rig.update(covariance(r, S, pose_covariance_rig_into, (ext, estride), cameras, count, r["pose"], r["result"]))
            # per image: the frame form at E_c o rig pose on the image's own rows
            per.update(covariance(b, B, pose_covariance_batch_into, count, b["pose"], b["result"]))
        return per, K, rig


def pose_nees(pose, P_gt, info: torch.Tensor, stat: torch.Tensor) -> torch.Tensor:
    """Normalised estimation error squared of B poses against ground truth (cofi_pose_nees): e = (log(R_gt R_est^T), t_gt - exp(omega)
    t_est), nees = e^T info e - chi-square with 6 degrees of freedom for a calibrated covariance; NaN where stat[:, 0] == 0.  pose (B,12)
    or (R, t); P_gt (B,4,4) float64 or float32 in the direction of the pose, as pose_errors takes it; info (B,6,6), stat (B,4) of
    pose_covariance*.  Returns a (B,) float64 device tensor; nothing is synchronised."""
    lib = _lib.load()
    what = "pose_nees"
    if not (torch.is_tensor(info) and info.is_cuda and info.dtype == torch.float64 and info.dim() == 3 and tuple(info.shape[1:]) == (6, 6)
            and info.is_contiguous() and info.shape[0] >= 1):
        raise _lib.CofiError("%s: info must be a contiguous CUDA float64 (B,6,6) tensor with B >= 1" % what)
    B, dev = info.shape[0], info.device
    if not (torch.is_tensor(stat) and stat.is_cuda and stat.device == dev and stat.dtype == torch.float64 and tuple(stat.shape) == (B, 4)
            and stat.is_contiguous()):
        raise _lib.CofiError("%s: stat must be a contiguous CUDA float64 (%d,4) tensor" % (what, B))
    pose = _pose12(pose, B, what)
    if not torch.is_tensor(P_gt):
        P_gt = torch.as_tensor(np.asarray(P_gt))
    if tuple(P_gt.shape) != (B, 4, 4) or P_gt.dtype not in (torch.float64, torch.float32):
        raise _lib.CofiError("%s: P_gt must be a (%d,4,4) float64 or float32 tensor" % (what, B))
    P_gt = P_gt.to(dev, non_blocking=True).contiguous()
    out = torch.empty(B, dtype=torch.float64, device=dev)
    _lib.check(lib.cofi_pose_nees(ops._p(pose), ops._p(P_gt), 1 if P_gt.dtype == torch.float64 else 0, ops._p(info), ops._p(stat), B, ops._p(out),
                                  ops._stream()), "cofi_pose_nees")
    return out


def _skew(t):
    z = torch.zeros((), dtype=t.dtype, device=t.device)
    return torch.stack([torch.stack([z, -t[2], t[1]]), torch.stack([t[2], z, -t[0]]), torch.stack([-t[1], t[0], z])])


def transport_covariance(cov: torch.Tensor, E) -> torch.Tensor:
    """The covariance of a camera's pose E_c o T from the rig's (float64 torch): a perturbation (omega, v) of T perturbs E_c o T by
    (R_c omega, [t_c]x R_c omega + R_c v), so Sigma_c = A Sigma A^T with A = [[R_c, 0], [[t_c]x R_c, R_c]].  cov (6,6) or (S,6,6); E (3,4) /
    (4,4), camera <- rig, tensor or array."""
    cov = torch.as_tensor(cov).to(torch.float64)
    E = torch.as_tensor(np.asarray(E, dtype=np.float64) if not torch.is_tensor(E) else E).to(device=cov.device, dtype=torch.float64)
    if tuple(cov.shape[-2:]) != (6, 6) or tuple(E.shape) not in ((3, 4), (4, 4)):
        raise _lib.CofiError("transport_covariance: cov (..,6,6) and E (3,4) or (4,4), got %s and %s" % (tuple(cov.shape), tuple(E.shape)))
    Rc, tc = E[:3, :3], E[:3, 3]
    A = torch.zeros((6, 6), dtype=torch.float64, device=cov.device)
    A[:3, :3], A[3:, 3:], A[3:, :3] = Rc, Rc, _skew(tc) @ Rc
    out = A @ cov @ A.T
    return 0.5 * (out + out.transpose(-1, -2))


def covariance_sigmas(cov: torch.Tensor):
    """(rotation 1-sigma in degrees = sqrt(trace(Sigma_omega omega)) 180 / pi, translation 1-sigma in the units of the cloud =
    sqrt(trace(Sigma_vv))) of a covariance (6,6) or (..,6,6)"""
    d = torch.diagonal(torch.as_tensor(cov).to(torch.float64), dim1=-2, dim2=-1)
    return torch.sqrt(d[..., :3].sum(-1)) * (180.0 / np.pi), torch.sqrt(d[..., 3:].sum(-1))


def euler_xzy_deg(Rm: np.ndarray) -> np.ndarray:
    """scipy's Rotation.from_matrix(Rm).as_euler('xzy', degrees=True) (eval_all.py:20-21) without scipy: R = Ry(c) Rz(b) Rx(a)."""
    b = np.arcsin(np.clip(Rm[1, 0], -1.0, 1.0))
    if abs(Rm[1, 0]) < 1 - 1e-12:
        a = np.arctan2(-Rm[1, 2], Rm[1, 1])
        c = np.arctan2(-Rm[2, 0], Rm[0, 0])
    else:  # gimbal lock: third angle set to zero, as scipy does
        a = np.arctan2(Rm[2, 1], Rm[2, 2])
        c = 0.0
    return np.degrees(np.array([a, b, c]))


def get_P_diff(P_pred_np: np.ndarray, P_gt_np: np.ndarray):
    """eval_all.py:16-22: (t_diff, angles_diff) = (RTE, RRE) of inv(P_pred) @ P_gt."""
    P_diff = np.dot(np.linalg.inv(P_pred_np), P_gt_np)
    t_diff = np.linalg.norm(P_diff[0:3, 3])
    angles_diff = np.sum(np.abs(euler_xzy_deg(P_diff[0:3, 0:3])))
    return t_diff, angles_diff


def pose_matrix(R: torch.Tensor, t: torch.Tensor) -> np.ndarray:
    """T_pred of eval_all.py:111-113."""
    T = np.eye(4)
    T[0:3, 0:3] = R.detach().cpu().numpy().astype(np.float64)
    T[0:3, 3] = t.detach().cpu().numpy().astype(np.float64)
    return T
