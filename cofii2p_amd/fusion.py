"""Registered clouds: what a solved pose is for - image content attached to points and LiDAR depth attached to pixels.

    buffers = fuse(points, images, pose, K, cameras=C)         # cofi_fuse_cloud_image: four launches, no host sync
    buffers.depth   (F,H,W) float32   z of the nearest point that falls on the pixel (0 where empty)
    buffers.index   (F,H,W) int32     its cloud-local id (-1 where empty)
    buffers.flags   (F,N)   uint8     bit 0: the point is in the picture of image f, bit 1: and not hidden behind a nearer surface
    buffers.color   (S,N,Ci) float32  the image sampled at the point's projection in the camera that sees it most centrally (0: unseen)
    buffers.camera  (S,N)   int32     that camera (-1: unseen)
    buffers.stats   (F,4)   int32     [in picture, visible, pixels hit, 0]

The reference has only offline numpy helpers for this (data/kitti_helper.py:166-190 crop_pc_with_img, :142-163 projection_pc_img), without an
occlusion test and not reachable from a solved pose; the contract is in include/cofi_hip.h.  F = S * C images, image f looks at cloud
f // C - the layout of a stack-mode (C = 1) or rig (C > 1) submission, whose pose tail leaves exactly the operands this reads:
`forward_async(..., pose_K=K, fuse_into=buffers)` enqueues the fusion behind it, `serving.FrameBatcher(pose=True, fuse=True)` per stack."""
from typing import Optional

import numpy as np
import torch

from . import _lib, ops

class FusionBuffers:
    """The static outputs and the z-buffer workspace of one fusion: S clouds of N points, F images (Ci, H, W), F a multiple of S."""

    def __init__(self, S: int, N: int, F: int, H: int, W: int, Ci: int = 3, device="cuda"):
        S, N, F, H, W, Ci = (int(v) for v in (S, N, F, H, W, Ci))
        if min(S, N, F, H, W, Ci) < 1 or F % S:
            raise _lib.CofiError("FusionBuffers: need S, N, F, H, W, Ci >= 1 and F a multiple of S, got %s" % ((S, N, F, H, W, Ci),))
        need = _lib.load().cofi_fuse_workspace(F, H, W)
        if need == 0 or N > 0x7FFFFFFF:
            raise _lib.CofiError("FusionBuffers: N = %d or F * H * W = %d * %d * %d is beyond 31 bits" % (N, F, H, W))
        self.S, self.N, self.F, self.H, self.W, self.Ci = S, N, F, H, W, Ci
        dev = torch.device(device)
        self.depth = torch.zeros((F, H, W), dtype=torch.float32, device=dev)
        self.index = torch.full((F, H, W), -1, dtype=torch.int32, device=dev)
        self.flags = torch.zeros((F, N), dtype=torch.uint8, device=dev)
        self.color = torch.zeros((S, N, Ci), dtype=torch.float32, device=dev)
        self.camera = torch.full((S, N), -1, dtype=torch.int32, device=dev)
        self.stats = torch.zeros((F, 4), dtype=torch.int32, device=dev)
        self.ws = torch.empty(need // 8, dtype=torch.int64, device=dev)   # 8-byte aligned keys
        self.K = None   # (F,3,3) device copy of a host K, made on first use

    @property
    def device(self):
        return self.depth.device

    def fits(self, S, N, F, H, W, Ci, device) -> bool:
        return (self.S, self.N, self.F, self.H, self.W, self.Ci) == (S, N, F, H, W, Ci) and self.device == torch.device(device)


def _pose_rows(pose, F, what):
    """(F,12) rows [R | t] read in place -> (tensor whose data_ptr is row 0, row stride in floats).  A dict / pair (R (F,3,3), t (F,3)) that
    are the views handle["pose"] holds of one (F,12) buffer is read in place too; any other pair is joined into a new buffer."""
    E = _lib.CofiError
    if isinstance(pose, dict):
        pose = (pose["R"], pose["t"])
    if isinstance(pose, (tuple, list)):
        R, t = pose
        if not (torch.is_tensor(R) and torch.is_tensor(t) and tuple(R.shape) == (F, 3, 3) and tuple(t.shape) == (F, 3)
                and R.dtype == torch.float32 and t.dtype == torch.float32 and R.is_cuda and t.is_cuda and R.device == t.device):
            raise E("%s: a pose pair must be CUDA float32 R (F,3,3) and t (F,3) with F = %d" % (what, F))
        if (R.stride(1), R.stride(2), t.stride(1)) == (3, 1, 1) and (F == 1 or (R.stride(0) == t.stride(0) and R.stride(0) >= 12)) \
                and t.data_ptr() == R.data_ptr() + 36:
            return R, (R.stride(0) if F > 1 else 12)
        pose = torch.cat([R.reshape(F, 9), t], 1)
    if not (torch.is_tensor(pose) and pose.is_cuda and pose.dtype == torch.float32 and tuple(pose.shape) == (F, 12) and pose.stride(1) == 1
            and (F == 1 or pose.stride(0) >= 12)):
        raise E("%s: pose must be a CUDA float32 (F,12) = (%d,12) tensor with unit column stride and a row stride >= 12 (a view of a larger "
                "buffer is read in place), or the pair / dict of R (F,3,3) and t (F,3)" % (what, F))
    return pose, (pose.stride(0) if F > 1 else 12)


def _operands(points, images, pose, K, buffers, result, cameras, k_scale, z_near, splat, rel_tol, abs_tol, what="fuse_into"):
    """every check of fuse_into, before anything is enqueued -> the arguments of the library call"""
    E = _lib.CofiError
    if not isinstance(buffers, FusionBuffers):
        raise E("%s: buffers must be a FusionBuffers" % what)
    if not isinstance(cameras, int) or cameras < 1:
        raise E("%s: cameras must be an integer >= 1, got %r" % (what, cameras))
    if not (torch.is_tensor(images) and images.is_cuda and images.dtype == torch.float32 and images.dim() == 4 and images.is_contiguous()):
        raise E("%s: images must be a contiguous CUDA float32 (F,Ci,H,W) tensor" % what)
    F, Ci, H, W = images.shape
    dev = images.device
    if F < 1 or F % cameras:
        raise E("%s: F = %d images are no whole number of clouds under C = %d cameras" % (what, F, cameras))
    S = F // cameras
    if not (torch.is_tensor(points) and points.is_cuda and points.device == dev and points.dtype == torch.float32 and points.is_contiguous()
            and points.dim() in (2, 3) and points.shape[-1] == 3 and points.numel() > 0 and (points.numel() // 3) % S == 0
            and (points.dim() == 2 or points.shape[0] == S)):
        raise E("%s: points must be a contiguous CUDA float32 (S*N,3) or (S,N,3) tensor on the device of the images, S = F / C = %d" % (what, S))
    N = points.numel() // 3 // S
    if not buffers.fits(S, N, F, H, W, Ci, dev):
        raise E("%s: the buffers were made for (S,N,F,H,W,Ci) = %s on %s, the operands are %s on %s"
                % (what, (buffers.S, buffers.N, buffers.F, buffers.H, buffers.W, buffers.Ci), buffers.device, (S, N, F, H, W, Ci), dev))
    pose, pstride = _pose_rows(pose, F, what)
    if pose.device != dev:
        raise E("%s: pose must be on the device of the images" % what)
    rstride = 0
    if result is not None:
        if not (torch.is_tensor(result) and result.is_cuda and result.device == dev and result.dtype == torch.int32 and result.dim() in (1, 2)
                and result.shape[0] == F and result.numel() >= F and (F == 1 or result.stride(0) >= 1)):
            raise E("%s: result must be an int32 CUDA tensor (F,) or (F,k) whose column 0 is read (a strided view is read in place)" % what)
        rstride = max(1, result.stride(0))
    if not torch.is_tensor(K):
        K = torch.as_tensor(np.asarray(K, dtype=np.float32))
    if tuple(K.shape) not in ((F, 3, 3), (3, 3)):
        raise E("%s: K must be (F,3,3) = %s or (3,3), got %s" % (what, (F, 3, 3), tuple(K.shape)))
    try:
        scal = (float(k_scale), float(z_near), float(rel_tol), float(abs_tol))
    except (TypeError, ValueError):
        raise E("%s: k_scale, z_near, rel_tol and abs_tol must be numbers" % what)
    if not (scal[0] > 0.0 and scal[1] > 0.0 and scal[2] >= 0.0 and scal[3] >= 0.0 and all(np.isfinite(scal))):
        raise E("%s: need k_scale > 0, z_near > 0 (the keys order positive depths), rel_tol >= 0, abs_tol >= 0, all finite; got %s" % (what, scal))
    if not isinstance(splat, int) or not 0 <= splat <= 3:
        raise E("%s: splat must be an integer 0...3, got %r" % (what, splat))
    return S, N, F, H, W, Ci, points, pose, pstride, result, rstride, K, scal


def fuse_into(points, images, pose, K, buffers: FusionBuffers, result: Optional[torch.Tensor] = None, cameras: int = 1,
              k_scale: float = 1.0, z_near: float = 0.5, splat: int = 1, rel_tol: float = 0.02, abs_tol: float = 0.05) -> FusionBuffers:
    """The fusion into caller-owned buffers (cofi_fuse_cloud_image), on the current stream: four kernels, nothing else - no
    host synchronisation, capturable in a hipGraph.  Every operand is read in place:

    points (S*N,3) or (S,N,3) float32; images (F,Ci,H,W) float32, F = S * cameras, image f looks at cloud f // cameras; pose (F,12)
    [R row-major | t], camera <- cloud - possibly a view with a row stride >= 12 - or the pair / dict of R (F,3,3) and t (F,3) a forward
    handle holds in handle["pose"]; result (optional) int32 (F,) or (F,k), possibly strided: an image with result[f, 0] == 0 contributes
    nothing (its maps are empty, its flags 0); K (F,3,3) or (3,3): a contiguous float32 device (F,3,3) is read in place, anything else is
    copied into a buffer `buffers` owns; fx, fy, cx, cy are multiplied by k_scale (a half-resolution K with k_scale = 2 serves the full image).
    z_near: nearest depth kept; splat 0...3: every point covers the (2 splat + 1)^2 pixels around its own in the z-buffer; visible = in
    picture and z <= zmin * (1 + rel_tol) + abs_tol at its own pixel.  Anything unfit raises _lib.CofiError before a launch."""
    lib = _lib.load()
    S, N, F, H, W, Ci, points, pose, pstride, result, rstride, K, scal = _operands(points, images, pose, K, buffers, result, cameras, k_scale,
                                                                                  z_near, splat, rel_tol, abs_tol)
    b = buffers
    if not (K.is_cuda and K.device == b.device and K.dtype == torch.float32 and K.dim() == 3 and K.is_contiguous()):
        if b.K is None:
            b.K = torch.empty((F, 3, 3), dtype=torch.float32, device=b.device)
        b.K.copy_(K, non_blocking=True)   # broadcasts a (3,3)
        K = b.K
    rc = lib.cofi_fuse_cloud_image(ops._p(points), N, F, int(cameras), ops._p(images), Ci, H, W, ops._p(pose), int(pstride), ops._p(result),
                                   int(rstride), ops._p(K), scal[0], scal[1], int(splat), scal[2], scal[3], ops._p(b.ws), b.ws.numel() * 8,
                                   ops._p(b.depth), ops._p(b.index), ops._p(b.flags), ops._p(b.color), ops._p(b.camera), ops._p(b.stats),
                                   ops._stream())
    _lib.check(rc, "cofi_fuse_cloud_image")
    return b


def fuse(points, images, pose, K, result: Optional[torch.Tensor] = None, cameras: int = 1, k_scale: float = 1.0, z_near: float = 0.5,
         splat: int = 1, rel_tol: float = 0.02, abs_tol: float = 0.05) -> FusionBuffers:
    """fuse_into with buffers made for the operands; returns them."""
    E = _lib.CofiError
    if not (torch.is_tensor(images) and images.dim() == 4 and torch.is_tensor(points) and points.dim() in (2, 3) and points.shape[-1] == 3):
        raise E("fuse: points (S*N,3) / (S,N,3) and images (F,Ci,H,W) must be tensors")
    if not isinstance(cameras, int) or cameras < 1 or images.shape[0] < 1 or images.shape[0] % cameras:
        raise E("fuse: F = %d images are no whole number of clouds under cameras = %r" % (images.shape[0], cameras))
    if not images.is_cuda:
        raise E("fuse: images must be a CUDA tensor")
    F, Ci, H, W = images.shape
    S = F // cameras
    rows = points.numel() // 3
    if rows < S or rows % S:
        raise E("fuse: %d point rows are no whole number of S = %d clouds" % (rows, S))
    b = FusionBuffers(S, rows // S, F, H, W, Ci, images.device)
    return fuse_into(points, images, pose, K, b, result, cameras, k_scale, z_near, splat, rel_tol, abs_tol)
