"""Surface normals of a raw point cloud on the device (csrc/normals.hip: cofi_estimate_normals): what a KITTI-trained model expects in
three of its four point features (feats = [intensity | normal], data/kitti.py:293) and the reference only ever reads from its
pc_npy_with_normal file (kitti.py:130).  A velodyne .bin or a live scan carries no normal: this module computes it.

The defaults - k = 30 nearest neighbours, no radius, orientation towards the sensor at the origin - are this project's choice; the upstream
preprocessing uses a third-party point-cloud library and parity with it is unpinned."""
import operator
from typing import Optional

import torch

from . import _lib, ops

K_MAX = 128   # the k-nearest grid's widest row


def _p(t):
    return None if t is None else t.data_ptr()


def _check_points(points):
    if not torch.is_tensor(points) or not points.is_cuda or points.dtype != torch.float32 or points.dim() != 2 or points.shape[1] != 3 \
            or not points.is_contiguous():
        raise _lib.CofiError("normals: points must be contiguous CUDA float32 (n,3)")


def _check_k(k):
    """-> k as a Python int (numpy integers included); CofiError unless it is an integer in 1..K_MAX"""
    try:
        k = None if isinstance(k, bool) else operator.index(k)
    except TypeError:
        k = None
    if k is None or not 1 <= k <= K_MAX:
        raise _lib.CofiError("normals: k must be an integer in 1..%d" % K_MAX)
    return k


def normals_from_rows(points, idx, dist=None, k: Optional[int] = None, radius: Optional[float] = None, viewpoint=(0.0, 0.0, 0.0),
                      out: Optional[torch.Tensor] = None, degenerate_count: Optional[torch.Tensor] = None):
    """The kernel alone, on neighbour rows that exist already: idx (Q, ldi) int32 rows into points (row q = neighbourhood of point q), dist
    (Q, ldi) squared distances (needed with a radius), k <= ldi slots of each row read (default: all).  viewpoint: three numbers, a CUDA
    float32 tensor of 3, or None (unoriented: largest component positive).  out: any float32 CUDA view of shape (Q, 3) - e.g.
    `scan7n[4:7].t()` writes rows 4..6 of a channel-major scan in place.  degenerate_count: CUDA int32 (1,), zeroed by the caller.
    Enqueues one launch on the current stream; no host sync."""
    lib = _lib.load()
    _check_points(points)
    if not torch.is_tensor(idx) or not idx.is_cuda or idx.dtype != torch.int32 or idx.dim() != 2 or idx.stride(1) != 1 or idx.stride(0) < idx.shape[1]:
        raise _lib.CofiError("normals: idx must be CUDA int32 (q,ldi) with unit column stride")
    Q, ldi = idx.shape[0], idx.stride(0)
    k = _check_k(idx.shape[1] if k is None else k)
    if k > idx.shape[1]:
        raise _lib.CofiError("normals: k = %d exceeds the %d slots of a neighbour row" % (k, idx.shape[1]))
    if Q > points.shape[0]:
        raise _lib.CofiError("normals: %d neighbour rows for %d points (row q belongs to point q)" % (Q, points.shape[0]))
    if dist is not None and (not torch.is_tensor(dist) or not dist.is_cuda or dist.dtype != torch.float32 or dist.shape != idx.shape
                             or dist.stride() != idx.stride()):
        raise _lib.CofiError("normals: dist must be CUDA float32 with the shape and strides of idx")
    if radius is not None and radius > 0 and dist is None:
        raise _lib.CofiError("normals: a radius needs the squared distances of the neighbour rows")
    if out is None:
        out = torch.empty((Q, 3), dtype=torch.float32, device=points.device)
    elif not torch.is_tensor(out) or not out.is_cuda or out.dtype != torch.float32 or tuple(out.shape) != (Q, 3) or (Q > 0 and 0 in out.stride()):
        raise _lib.CofiError("normals: out must be a CUDA float32 view of shape (%d,3)" % Q)
    if degenerate_count is not None and (not degenerate_count.is_cuda or degenerate_count.dtype != torch.int32 or degenerate_count.numel() < 1):
        raise _lib.CofiError("normals: degenerate_count must be a CUDA int32 tensor")
    if torch.is_tensor(viewpoint):
        if not viewpoint.is_cuda or viewpoint.dtype != torch.float32 or viewpoint.numel() != 3 or not viewpoint.is_contiguous():
            raise _lib.CofiError("normals: a viewpoint tensor must be contiguous CUDA float32 of 3 elements")
        vp = viewpoint
    elif viewpoint is not None:
        if len(viewpoint) != 3:
            raise _lib.CofiError("normals: the viewpoint is three coordinates (or None for unoriented normals)")
        vp = _viewpoint_dev(tuple(float(v) for v in viewpoint), points.device)
    else:
        vp = None
    if Q == 0:
        return out
    _lib.check(lib.cofi_estimate_normals(_p(points), points.shape[0], _p(idx), _p(dist), Q, k, ldi, float(radius) if radius else 0.0, _p(vp),
                                         _p(out), out.stride(0), out.stride(1), _p(degenerate_count), torch.cuda.current_stream().cuda_stream),
               "cofi_estimate_normals")
    return out


_VIEWPOINTS = {}


def _viewpoint_dev(v, device):
    """three host numbers -> a cached device tensor (the origin, in practice: no upload per frame)"""
    key = (v, str(device))
    t = _VIEWPOINTS.get(key)
    if t is None:
        if len(_VIEWPOINTS) >= 64:
            _VIEWPOINTS.clear()
        t = _VIEWPOINTS[key] = torch.tensor(v, dtype=torch.float32, device=device)
    return t


def estimate_normals(points: torch.Tensor, k: int = 30, radius: Optional[float] = None, viewpoint=(0.0, 0.0, 0.0),
                     out: Optional[torch.Tensor] = None, return_degenerate: bool = False, grid: Optional[ops.KnnGrid] = None):
    """points (N, 3) contiguous CUDA float32 -> unit normals (N, 3): the k nearest points of every point (itself included; with `radius`
    only those within it), covariance, eigenvector of the smallest eigenvalue, oriented towards `viewpoint` (None: unoriented).  Rows with
    fewer than 3 neighbours or coincident neighbours get (0, 0, 1).  grid: a KnnGrid of `points` with its order (built here when None).
    Grid build + self search in cell order + one kernel on the current stream; no host sync unless return_degenerate=True, which returns
    (normals, number of degenerate rows)."""
    _check_points(points)
    k = _check_k(k)
    if radius is not None and not radius > 0:
        raise _lib.CofiError("normals: radius must be positive (None for no radius)")
    N = points.shape[0]
    if N == 0:
        res = torch.empty((0, 3), dtype=torch.float32, device=points.device) if out is None else out
        return (res, 0) if return_degenerate else res
    if grid is None:
        grid = ops.KnnGrid(points)
    elif grid.S != N or grid.support.data_ptr() != points.data_ptr():
        raise _lib.CofiError("normals: the grid was built over another point set")
    if radius is not None:
        idx, dist = grid.search(points, k, return_dist=True, qorder=grid.order)
    else:   # no radius: the distance table (4 k bytes per point) is neither written nor read
        idx, dist = grid.search(points, k, qorder=grid.order), None
    count = torch.zeros(1, dtype=torch.int32, device=points.device) if return_degenerate else None
    res = normals_from_rows(points, idx, dist, k, radius, viewpoint, out, count)
    return (res, int(count.item())) if return_degenerate else res
