"""The evaluation pass of the reference on the device: evaluation/eval_all.py:63-139 followed by IR_RMSE.py and calc_result.py, without
the per-frame host round trips and result files.

What the reference's caller loop does per frame - read R, t back, `get_P_diff` in numpy, pickle a dict of 10 240 points, and later
re-read every file 51 times for the inlier ratio - is one small kernel here, `cofi_eval_monitors` (csrc/evaluation.hip): one launch per
stack-mode submission behind its pose tail, reading the submission's coarse points, coordinate-major fine_xy, device-side counts, poses
and camera matrices in place, and writing one float64 row per frame into a device table.  The table is copied to the host once.

    res = evaluate(model, samples, opt)                       # samples: FrameLoader.complete / the reference's DataLoader batches of 1
    print("\\n".join(res["report"]))                           # calc_result.py's text
    res["ir_curve"], res["rmse"]                              # IR_RMSE.py's inlier-ratio curve and per-frame "RMSE"

A row of the table (6 + T float64 columns, T = number of pixel thresholds):

    0 n | 1 success | 2 inliers | 3 RTE | 4 RRE | 5 mean residual ("RMSE") | 6 .. 5+T  number of residuals <= thresholds[i]

RTE / RRE are NaN for a frame whose pose failed (the reference appends nothing for such a frame; its `pred_P` then repeats the previous
frame's pose in the result file - that reuse is not reproduced), the mean residual is NaN for a frame without matches.  `metrics.py`
keeps its role for result files; `evaluate(result_dir=...)` still writes them."""
from typing import Dict, Iterable, Optional

import numpy as np
import torch

from . import _lib, metrics, ops
from .pose import image_points

__all__ = ["EvalTable", "eval_monitors", "summarize", "evaluate", "ROW_COLUMNS"]

ROW_COLUMNS = ("n", "success", "inliers", "rte", "rre", "rmse")   # then one count per threshold


class EvalTable:
    """The device table `cofi_eval_monitors` writes: rows (rows, 6 + T) float64, pre-filled with NaN (a row no frame wrote stays NaN),
    and the device copy of the T pixel thresholds (default: metrics.pixel_thresholds(), 0 .. 10 step 0.2)."""

    def __init__(self, rows: int, thresholds=None, device="cuda"):
        thr = metrics.pixel_thresholds() if thresholds is None else np.asarray(thresholds, dtype=np.float64)
        if thr.ndim != 1 or thr.shape[0] < 1:
            raise _lib.CofiError("EvalTable: thresholds must be a 1-D array of at least one value")
        if int(rows) < 1:
            raise _lib.CofiError("EvalTable: need at least one row")
        dev = torch.device(device)
        if dev.type != "cuda":
            raise _lib.CofiError("EvalTable lives on the GPU - there is no CPU path")
        self.thresholds_host = thr.copy()
        self.thresholds = torch.from_numpy(self.thresholds_host).to(dev)
        self.rows = torch.full((int(rows), len(ROW_COLUMNS) + thr.shape[0]), float("nan"), dtype=torch.float64, device=dev)

    @property
    def device(self):
        return self.rows.device

    def host(self) -> np.ndarray:
        """the table as a numpy array: the one device-to-host copy of an evaluation (synchronises the current stream)"""
        return self.rows.cpu().numpy()


def _pose12(pose) -> torch.Tensor:
    """handle["pose"] / (R, t) / (B,12) -> the (B,12) float32 buffer; R and t as the batched solver returns them are views of one"""
    if isinstance(pose, dict):
        pose = (pose["R"], pose["t"])
    if isinstance(pose, (tuple, list)):
        R, t = pose
        if not (torch.is_tensor(R) and torch.is_tensor(t) and R.dim() == 3 and tuple(R.shape[1:]) == (3, 3) and tuple(t.shape) == (R.shape[0], 3)):
            raise _lib.CofiError("eval_monitors: (R, t) must be (B,3,3) and (B,3) tensors")
        B = R.shape[0]
        if (R.dtype == t.dtype == torch.float32 and R.stride() == (12, 3, 1) and t.stride() == (12, 1)
                and t.data_ptr() == R.data_ptr() + 36 and R.untyped_storage().data_ptr() == t.untyped_storage().data_ptr()):
            return R.as_strided((B, 12), (12, 1))   # the solver's own buffer, in place
        return torch.cat([R.reshape(B, 9), t], 1).contiguous()
    return pose


def _device_tensor(x, dev, dtype=None) -> torch.Tensor:
    if not torch.is_tensor(x):
        x = torch.as_tensor(np.asarray(x))
    if dtype is not None and x.dtype != dtype:
        x = x.to(dtype)
    return x.to(dev, non_blocking=True).contiguous()


def eval_monitors(handle_or_operands, K, P_gt, table: EvalTable, row_index=None) -> torch.Tensor:
    """One `cofi_eval_monitors` launch on the current stream, with no host read: frame f of the submission writes row row_index[f] of
    `table` (a negative index: nothing).

    handle_or_operands: a `CoFiI2P.forward_async(..., pose_K=...)` handle (its coarse points, coordinate-major fine_xy, counts and poses
    are read in place), or the raw tensors as a dict {"object_points" (B,cap,3), "image_points" (B,cap,2) - (B,2,cap) with "coord_major":
    True -, "count" (int32 (B,), may be a strided view; absent = every row), "pose" ((B,12), or (R, t)), "result" (B,3) int32}.
    K (B,3,3) or (3,3); P_gt (B,4,4) float64 or float32; row_index (B,) int32 (None: frame f -> row f).  Host arrays are uploaded;
    float32 / int32 device tensors are read in place.  Returns table.rows."""
    if not isinstance(table, EvalTable):
        raise _lib.CofiError("eval_monitors: table must be an EvalTable")
    if not isinstance(handle_or_operands, dict):
        raise _lib.CofiError("eval_monitors: pass a forward_async handle or a dict of operands")
    h = handle_or_operands
    if "out" in h:
        if "pose" not in h:
            raise _lib.CofiError("eval_monitors: the handle carries no pose - submit with forward_async(..., pose_K=...)")
        o0 = h["out"][0]
        if "coarse_pts_all" not in o0:
            raise _lib.CofiError("eval_monitors reads the submission-wide outputs of match_finish (coarse_pts_all, ...)")
        obj, img, count, coord_major = o0["coarse_pts_all"], image_points(h["out"]), o0["count_all"][:, 0], True
        pose, result = _pose12(h["pose"]), h["pose"]["result"]
    else:
        missing = [k for k in ("object_points", "image_points", "pose", "result") if k not in h]
        if missing:
            raise _lib.CofiError("eval_monitors: operands lack %s" % missing)
        obj, img, count, coord_major = h["object_points"], h["image_points"], h.get("count"), bool(h.get("coord_major", False))
        pose, result = _pose12(h["pose"]), h["result"]
    if not (torch.is_tensor(obj) and obj.is_cuda and obj.dim() == 3):
        raise _lib.CofiError("eval_monitors: object_points must be a CUDA (B,cap,3) tensor - there is no CPU path")
    B, dev = obj.shape[0], obj.device
    if table.device != dev:
        raise _lib.CofiError("eval_monitors: the table is on %s, the operands on %s" % (table.device, dev))
    K = _device_tensor(K, dev, torch.float32)
    if tuple(K.shape) == (3, 3):
        K = K.expand(B, 3, 3).contiguous()
    P_gt = _device_tensor(P_gt, dev) if torch.is_tensor(P_gt) and P_gt.dtype in (torch.float64, torch.float32) else _device_tensor(P_gt, dev, torch.float64)
    if tuple(P_gt.shape) == (4, 4):
        P_gt = P_gt.expand(B, 4, 4).contiguous()
    row_index = torch.arange(B, dtype=torch.int32, device=dev) if row_index is None else _device_tensor(row_index, dev, torch.int32)
    if not torch.is_tensor(pose):
        raise _lib.CofiError("eval_monitors: pose must be a (B,12) tensor or a pair (R, t)")
    return ops.eval_monitors(obj, img, count, K, pose.contiguous(), result, P_gt, table.thresholds, row_index, table.rows, coord_major=coord_major)


def check_eval_into(eval_into, B: int, dev):
    """the `eval_into=(table, P_gt, row_index)` of forward_async, checked before anything is enqueued: device tensors read in place"""
    E = _lib.CofiError
    if not (isinstance(eval_into, (tuple, list)) and len(eval_into) == 3):
        raise E("forward_async: eval_into must be (table, P_gt, row_index)")
    table, P_gt, row_index = eval_into
    if not isinstance(table, EvalTable) or table.device != dev:
        raise E("forward_async: eval_into[0] must be an EvalTable on the device of the submission")
    if not (torch.is_tensor(P_gt) and P_gt.is_cuda and P_gt.device == dev and P_gt.dtype in (torch.float64, torch.float32)
            and tuple(P_gt.shape) == (B, 4, 4) and P_gt.is_contiguous()):
        raise E("forward_async: eval_into[1] (P_gt) must be a contiguous CUDA float64 or float32 (B,4,4) = %s tensor" % ((B, 4, 4),))
    if not (torch.is_tensor(row_index) and row_index.is_cuda and row_index.device == dev and row_index.dtype == torch.int32
            and tuple(row_index.shape) == (B,) and row_index.is_contiguous()):
        raise E("forward_async: eval_into[2] (row_index) must be a contiguous CUDA int32 (B,) = (%d,) tensor" % B)


def summarize(rows_host, thresholds=None) -> Dict[str, object]:
    """Pure numpy: the rows of an evaluation (one per frame, in frame order) -> what eval_all.py, IR_RMSE.py and calc_result.py report.

    n (frames,) int; success (frames,) bool; rte, rre (frames,) - NaN where the pose failed; t_error / r_error: the successful frames'
    RTE / RRE in frame order (what eval_all.py:138-139 saves); rmse (frames,) - NaN without matches; ir (frames, T) = count / n (NaN
    rows without matches); ir_curve (T,) = the mean of ir over the frames that have matches (IR_RMSE.py:68; NaN when none has);
    frames_without_matches: their indices; report: metrics.report(r_error, t_error) - calc_result.py's text."""
    thr = metrics.pixel_thresholds() if thresholds is None else np.asarray(thresholds, dtype=np.float64)
    rows = np.asarray(rows_host, dtype=np.float64)
    C = len(ROW_COLUMNS)
    if rows.ndim != 2 or rows.shape[1] != C + thr.shape[0]:
        raise ValueError("summarize: rows must be (frames, 6 + T) = (*, %d)" % (C + thr.shape[0]))
    if np.isnan(rows[:, :3]).any():
        raise ValueError("summarize: rows %s were never written" % np.nonzero(np.isnan(rows[:, :3]).any(1))[0].tolist())
    n = rows[:, 0].astype(np.int64)
    success = rows[:, 1] != 0
    rte, rre = rows[:, 3].copy(), rows[:, 4].copy()
    has = n > 0
    ir = np.full((rows.shape[0], thr.shape[0]), np.nan)
    ir[has] = rows[has, C:] / n[has, None].astype(np.float64)
    ir_curve = ir[has].mean(0) if has.any() else np.full(thr.shape[0], np.nan)
    t_error, r_error = rte[success], rre[success]
    return {"n": n, "success": success, "inliers": rows[:, 2].astype(np.int64), "rte": rte, "rre": rre, "t_error": t_error, "r_error": r_error,
            "rmse": rows[:, 5].copy(), "ir": ir, "ir_curve": ir_curve, "thresholds": thr.copy(),
            "frames_without_matches": np.nonzero(~has)[0], "report": metrics.report(r_error, t_error)}


def _sample_parts(sample: Dict, dev):
    """(pc_data_dict, img (1,3,H,W), K (3,3), P (4,4)) of a data-side sample; leading batch dimensions of 1 are squeezed (eval_all.py:70-78)"""
    sq = lambda t: torch.squeeze(t.to(dev), 0) if t.dim() and t.shape[0] == 1 else t.to(dev)
    pc = sample["pc_data_dict"]
    pyr = {k: [sq(t) for t in pc[k]] for k in ("points", "neighbors", "subsampling", "upsampling")}
    pyr["feats"] = sq(pc["feats"])
    if "order" in pc:
        pyr["order"] = [sq(t) for t in pc["order"]]
    img = sample["img"].to(dev)
    img = img[None] if img.dim() == 3 else img
    K, P = (torch.as_tensor(np.asarray(sample[k])) if not torch.is_tensor(sample[k]) else sample[k] for k in ("K", "P"))
    return pyr, img, K.reshape(3, 3), P.reshape(4, 4)


def _save_frame(fb, directory, step, ticket, pyr, K, P):
    """one result file of eval_all.py:121-131 for a frame the batcher has finished (per-frame device reads)"""
    from .pose import pose_matrix

    res, R, t, _ = fb.pose_result(ticket)
    try:
        out = fb.result(ticket)
        fine_xy, object_points, score = fb.fine_xy(ticket).cpu(), out[7].cpu(), out[3].cpu()
    except RuntimeError:   # no matches at any threshold: an empty frame
        fine_xy, object_points, score = torch.zeros((2, 0)), torch.zeros((0, 3)), torch.zeros((1, 1, 0))
    pred_P = pose_matrix(R, t)   # identity when the pose failed
    result = metrics.frame_result(P.detach().cpu().numpy(), pred_P, K.detach().cpu(), pyr["points"][1].cpu(), pyr["points"][-1].cpu(), score,
                                  fine_xy, object_points)
    if fb.subpixel:   # asked for: the points pred_P was fitted to, next to the reference's fine_xy
        result["sub_xy"] = fb.sub_xy(ticket).cpu() if fine_xy.shape[1] else torch.zeros((2, 0))
    metrics.save_frame_result(directory, step, result)


def evaluate(model, frames: Iterable[Dict], opt=None, batch: int = 16, streams: int = 4, pose_iterations: int = 10000,
             result_dir: Optional[str] = None, thresholds=None, slot_base: int = 200, device=None, subpixel: bool = False) -> Dict[str, object]:
    """eval_all.py:63-139 plus IR_RMSE.py and calc_result.py over `frames`: an iterable of data-side samples holding 'pc_data_dict', 'img',
    'K' (the camera matrix of the image the network sees) and 'P' (the reference's GT_P) - FrameLoader.complete samples, or batches of 1
    of the reference's DataLoader; equal sizes.  The frames go through `FrameBatcher(pose=True, eval_table=...)`: `batch` frames per
    stack-mode submission on `streams` streams, poses solved behind each forward with `pose_iterations` hypotheses, the monitors of a
    stack in one launch behind its poses; frame i lands in row i.  The module is put into eval() for the pass and back afterwards.
    ONE device-to-host copy, of the table, at the end.  -> the dict of `summarize`, plus "rows" (the host table).

    result_dir: additionally write the reference's per-frame result files (%06d.npy, metrics.save_frame_result) there; this reads
    every frame's points and matches back and is off by default.  `opt` is accepted for the shape of `validate`; nothing is read from it.
    subpixel=True: the pass runs on sub-pixel matches (FrameBatcher(subpixel=True), ops.fine_refine): poses, inlier ratios and residuals
    are those of the refined points, and the result files gain "sub_xy" (2, n) next to the unchanged "fine_xy".
    A frame's tensors must stay unmodified until its stack has been submitted (`FrameBatcher.submit`).  The batcher of a configuration
    (batch, streams, slot_base, pose_iterations) stays on the module with its ring of stacks, so a later pass replays the same captured
    graphs; `model._eval_batchers.clear()` lets go of them."""
    from .serving import FrameBatcher

    dev = torch.device(device) if device is not None else next(model.parameters()).device
    if not hasattr(frames, "__len__"):
        frames = list(frames)
    N = len(frames)
    if N == 0:
        raise ValueError("evaluate: no frame")
    table = EvalTable(N, thresholds, dev)
    was_training = model.training
    model.eval()
    try:
        # one batcher per configuration, kept on the module: its stacks are the static inputs of the slots' captured graphs, so a later
        # pass (the next epoch's evaluation) replays them instead of capturing new ones
        key = (int(batch), int(streams), int(slot_base), int(pose_iterations), str(dev)) + (("subpixel",) if subpixel else ())
        batchers = model.__dict__.setdefault("_eval_batchers", {})
        fb = batchers.get(key)
        if fb is None:
            fb = batchers[key] = FrameBatcher(model, batch=batch, streams=streams, slot_base=slot_base, pose=True, pose_iterations=pose_iterations,
                                              eval_table=table, subpixel=bool(subpixel))
        fb.reset()   # a pass that ended in an exception may have left a partly filled stack
        fb.eval_table = table
        prev, cur = [], []   # result files: the frames of a stack are written while the next stack runs
        for i, sample in enumerate(frames):
            pyr, img, K, P = _sample_parts(sample, dev)
            nsub = fb.submissions
            ticket = fb.submit(pyr, img, K, P_gt=P, row=i)
            if result_dir is not None:
                cur.append((i, ticket, pyr, K, P))
                if fb.submissions > nsub:   # this frame completed a stack
                    for args in prev:
                        _save_frame(fb, result_dir, *args)
                    prev, cur = cur, []
        fb.drain()
        for args in prev + cur:
            _save_frame(fb, result_dir, *args)
    finally:
        model.train(was_training)
    rows = table.host()   # the pass's only device-to-host copy
    res = summarize(rows, table.thresholds_host)
    res["rows"] = rows
    return res
