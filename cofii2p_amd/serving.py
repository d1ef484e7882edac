"""Single-frame API, stack-mode execution: a stream of independent frames served at the batch rates of the MI355X.

The reference evaluates one frame per `model(...)` call (`evaluation/eval_all.py:63-131`, `data/options.py:46` val_batch_size = 1).  On
MI355X one KITTI frame is a chain of ~250 dependent launches that cannot fill 256 CUs; B frames through the SAME launches (stack mode,
`CoFiI2P.stack_frames`) can: 480 frames/s with one frame per submission, 525 / 580 / 598 / 635 with 2 / 4 / 8 / 16 (bf16x6, DESIGN.md
section 12).  `FrameBatcher` keeps the caller's side at one frame per call:

    fb = FrameBatcher(model, batch=16)
    for pyr, img in frames:                 # device-resident pyramid dict (int32 or int64 tables) + (1, 3, H, W) image, equal sizes
        t = fb.submit(pyr, img)             # copies the frame into the stack being filled (one batched copy launch); returns at once
        ...
        out8 = fb.result(t)                 # the reference's 8-tuple of THAT frame (flushes a partly filled stack if it must)

Frames are copied into a ring of static stacks (`preprocess.FrameStack`); a full stack is submitted with
`forward_async(slot, stack.pyr, stack.img, inputs_stable=True)` on one of `streams` HIP streams, so the captured hipGraph of a slot reads the
stack in place and several submissions are in flight.  A partly filled stack is completed by repeating its last frame (results of the
padding are dropped): every submission has the one shape its graph was captured for.  Outputs are views of the slot's static buffers:
valid until the stack is reused, i.e. for the next `ring - 1` submissions - clone what must live longer.  Results are those of the
stack-mode forward (per-frame statistics, frame-local gathers: `tests/test_forward_gpu.py::test_stack_mode_batch_equals_single_frames`).

Frames in, poses out (`evaluation/eval_all.py:94-117` at batch rates): `FrameBatcher(model, pose=True)`, `submit(pyr, img, K)` with the
frame's (3,3) camera matrix, and `pose_result(t)` -> (result (3,) int32 [success, inliers, hypothesis], R (3,3), t (3,), inlier mask of the
frame's n matches): the poses of a whole stack are solved in one batched pass behind its forward (`forward_async(..., pose_K=...)`).

Frames in, evaluation rows out (`evaluation.evaluate`): `FrameBatcher(model, pose=True, eval_table=table)`, `submit(pyr, img, K, P_gt=...,
row=i)` with the frame's (4,4) ground-truth pose: the monitors of a stack (`evaluation.eval_monitors`, one launch) run behind its poses and
frame i lands in row i of the `evaluation.EvalTable`; padding frames write nothing.  `drain()` waits for everything submitted.

Rigs (one cloud under C images: the cameras around one sweep, a stereo pair): `FrameBatcher(model, batch=B, cameras=C)` with B a multiple
of C, and `submit_rig(pyr, imgs (C,3,H,W), K (C,3,3), P_gt (C,4,4), rows)` -> C tickets, one per image, used like the tickets of `submit`.
A stack then holds B // C clouds and B images and is submitted with `forward_async(..., cameras=C)`: the point encoder runs once per
cloud.  A partly filled stack is completed with copies of its last RIG.

Rig pose (the C cameras are bolted to one body: ONE pose per rig from the matches of all its cameras, `pose.solve_pnp_ransac_rig`):
`FrameBatcher(model, batch=B, cameras=C, pose=True, rig_extrinsics=E)` with E (C,4,4) / (C,3,4), camera <- rig (Y_cam = R_c Y_rig + t_c),
for every rig, or `rig_extrinsics="per_rig"` and `submit_rig(..., extrinsics=E)` with each rig's own (C,4,4) / (C,3,4).
`rig_pose_result(t)` -> (result (3,) int32 [success, inliers over all cameras, hypothesis], R (3,3), t (3,)) of the ticket's rig, rig <-
cloud; `pose_result(t)` stays per image and holds E_c o rig pose with that image's share of the consensus.

Registered clouds (`fusion.fuse_into` behind the pose tail of every stack): `FrameBatcher(model, pose=True, fuse=True[, cameras=C,
rig_extrinsics=E])`; `fusion_result(t)` -> {"depth" (H,W), "index" (H,W), "flags" (N,), "stats" (4,)} of the ticket's image plus "color"
(N,3) and "camera" (N,) of its cloud - with cameras = C the maps of all C images of the ticket's rig, (C,H,W) / (C,N) / (C,4).  One
`fusion.FusionBuffers` per stack of the ring, so the views live as long as `result(t)` does.

Pose uncertainty (`pose.pose_covariance_batch` / `pose_covariance_rig` behind the pose tail of every stack): `FrameBatcher(model, pose=True,
covariance=True[, sigma_px=...])`; `covariance_result(t)` -> (cov (6,6), info (6,6), stat (4,) = [ok, rows used, sigma_hat^2, min_pivot])
float64 of the pose of the ticket's image, `rig_covariance_result(t)` -> the same of its rig (with rig_extrinsics), in the tangent space
(omega, v) of the left-multiplied perturbation.  sigma_px: the 1-sigma pixel noise if it is known; None estimates it from the residuals.

Sub-pixel matches (`ops.fine_refine`, one launch inside every stack's recorded forward): `FrameBatcher(model, subpixel=True)`;
`sub_xy(t)` -> (2, n), column and row on the fine map, next to `fine_xy(t)`, which stays the reference's.  With `pose=True` the poses,
and everything behind them, are fitted to the sub-pixel points (INTEGRATION.md "Sub-pixel matches").
"""
from typing import Dict, List, Optional, Tuple

import torch

from .network import CoFiI2P
from .preprocess import FrameStack


class FrameBatcher:
    def __init__(self, model: CoFiI2P, batch: int = 16, streams: int = 4, ring: Optional[int] = None, slot_base: int = 200,
                 pose: bool = False, pose_iterations: int = 10000, eval_table=None, cameras: int = 1, rig_extrinsics=None,
                 fuse: bool = False, covariance: bool = False, sigma_px: Optional[float] = None, subpixel: bool = False):
        if batch < 1:
            raise ValueError("batch must be >= 1")
        if covariance and not pose:
            raise ValueError("FrameBatcher(covariance=True): the covariance belongs to the poses - pass pose=True")
        if sigma_px is not None and not covariance:
            raise ValueError("FrameBatcher(sigma_px=...): the pixel noise goes with covariance=True")
        if sigma_px is not None and not (float(sigma_px) > 0.0 and float(sigma_px) < float("inf")):
            raise ValueError("FrameBatcher(sigma_px=...): a finite number > 0, or None to estimate the pixel variance")
        self.covariance = bool(covariance)
        self._pose_cov = {} if not covariance else {"pose_cov": True if sigma_px is None else float(sigma_px)}
        self.subpixel = bool(subpixel)
        if fuse and not pose:
            raise ValueError("FrameBatcher(fuse=True): the fusion reads the poses - pass pose=True")
        if cameras < 1 or batch % cameras:
            raise ValueError("batch = %d is no whole number of rigs of cameras = %d" % (batch, cameras))
        self.model, self.B, self.C = model, int(batch), int(cameras)
        self.S = max(1, int(streams))
        self.ring = int(ring) if ring is not None else 2 * self.S     # stacks: one being filled + the ones in flight
        if self.ring < 2:
            raise ValueError("ring must hold at least two stacks")
        self.slot_base = slot_base
        self._streams: Optional[List[torch.cuda.Stream]] = None
        self._stacks: List[Optional[FrameStack]] = [None] * self.ring
        self._handles: List[Optional[Dict]] = [None] * self.ring     # forward_async handle of the stack's last submission
        self._results: List[Optional[list]] = [None] * self.ring     # finished 8-tuples of that submission
        self._serial = [0] * self.ring                               # submissions made from this stack: tickets of older ones are stale
        self._cur, self._fill = 0, 0                                 # stack being filled, frames in it
        self._last: Optional[Tuple[Dict, torch.Tensor]] = None
        self._nsub = 0
        self.pose, self.pose_iterations = bool(pose), int(pose_iterations)
        self._K: List[Optional[torch.Tensor]] = [None] * self.ring   # (B,3,3) device buffer of each stack: the frames' camera matrices
        self._poses: List[Optional[Dict]] = [None] * self.ring       # handle["pose"] of the stack's finished submission
        self._fine: List[Optional[list]] = [None] * self.ring        # per-frame fine matches (2, n) of that submission
        self._sub: List[Optional[list]] = [None] * self.ring         # per-frame sub-pixel matches (2, cap) of it (subpixel=True)
        self._counts: List[Optional[List[int]]] = [None] * self.ring  # matches per frame of that submission
        if eval_table is not None and not self.pose:
            raise ValueError("FrameBatcher(eval_table=...): the evaluation monitors read the poses - pass pose=True")
        self.eval_table = eval_table
        self._P: List[Optional[torch.Tensor]] = [None] * self.ring   # (B,4,4) float64 device buffer of each stack: the frames' ground-truth poses
        self._row: List[Optional[torch.Tensor]] = [None] * self.ring  # (B,) int32: the table row of each frame, -1 for padding
        # rig pose: one set of extrinsics for every rig (converted on first use, when the device is known), or a (S,C,12) buffer per stack
        self.rig = rig_extrinsics is not None
        self.rig_per_rig = isinstance(rig_extrinsics, str)
        if self.rig:
            if not self.pose or self.C == 1:
                raise ValueError("FrameBatcher(rig_extrinsics=...): the rig pose needs pose=True and cameras > 1")
            if self.rig_per_rig and rig_extrinsics != "per_rig":
                raise ValueError("FrameBatcher(rig_extrinsics=...): extrinsics (C,4,4) / (C,3,4), or 'per_rig' with submit_rig(extrinsics=...)")
            if not self.rig_per_rig:
                from . import pose as _pose

                rig_extrinsics = _pose.rig_extrinsics(rig_extrinsics, self.C, "cpu")   # checked here; uploaded once in _rig_ext
                if rig_extrinsics[0].dim() != 2:
                    raise ValueError("FrameBatcher(rig_extrinsics=...): one set of (C,4,4) / (C,3,4); per-rig sets go through 'per_rig'")
        self._ext_shared = None if self.rig_per_rig else rig_extrinsics
        self._ext: List[Optional[torch.Tensor]] = [None] * self.ring  # (S,C,12) device buffer of each stack (per-rig extrinsics)
        self._rig_poses: List[Optional[Dict]] = [None] * self.ring    # handle["rig_pose"] of the stack's finished submission
        self.fuse = bool(fuse)
        self._fusion: List[Optional[object]] = [None] * self.ring     # the stack's fusion.FusionBuffers, made at its first submission

    # ------------------------------------------------------------------ internals
    def _stream(self, j: int) -> torch.cuda.Stream:
        if self._streams is None:
            self._streams = self.model.frame_streams(self.S)
        return self._streams[j % self.S]

    def _collect(self, j: int):
        """read out the stack's pending submission.  A frame the model cannot serve (fewer than 4 coarse matches at every threshold -
        padding frames, copies of the last real one, can be such frames too) keeps its exception as ITS result: the other frames of the
        stack keep theirs, and the handle is cleared whatever happens, so one bad frame cannot wedge the ring."""
        h = self._handles[j]
        if h is None:
            return
        try:
            res = self.model.finish(h, per_frame_errors=True)
            self._results[j] = res if isinstance(res, list) else [res]
            self._poses[j] = h.get("pose")
            self._rig_poses[j] = h.get("rig_pose")
            self._fine[j] = h["fine_xy"]
            self._sub[j] = [o.get("sub_xy") for o in h["out"]]
            self._counts[j] = [max(0, int(n)) for n in h["count_host"][:, 0]]
        finally:
            self._handles[j] = None

    def _launch(self, j: int):
        st = self._stacks[j]
        rig = {} if self.C == 1 else {"cameras": self.C}
        if self.rig:
            rig["rig_extrinsics"] = self._rig_ext(j)
        if self.fuse:
            if self._fusion[j] is None:
                from . import fusion

                clouds = self.B // self.C
                self._fusion[j] = fusion.FusionBuffers(clouds, st.pyr["points"][0].shape[0] // clouds, self.B, st.img.shape[2], st.img.shape[3],
                                                       st.img.shape[1], st.img.device)
            rig["fuse_into"] = self._fusion[j]
        rig.update(self._pose_cov)
        if self.subpixel:
            rig["subpixel"] = True
        with torch.cuda.stream(self._stream(j)):
            if self.eval_table is not None:
                self._handles[j] = self.model.forward_async(self.slot_base + j, st.pyr, st.img, inputs_stable=True, pose_K=self._K[j],
                                                            pose_iterations=self.pose_iterations,
                                                            eval_into=(self.eval_table, self._P[j], self._row[j]), **rig)
            elif self.pose:
                self._handles[j] = self.model.forward_async(self.slot_base + j, st.pyr, st.img, inputs_stable=True, pose_K=self._K[j],
                                                            pose_iterations=self.pose_iterations, **rig)
            else:
                self._handles[j] = self.model.forward_async(self.slot_base + j, st.pyr, st.img, inputs_stable=True, **rig)
        self._results[j] = self._poses[j] = self._fine[j] = self._sub[j] = self._counts[j] = self._rig_poses[j] = None
        self._nsub += 1

    # ------------------------------------------------------------------ API
    def _put_K(self, j: int, f: int, K):
        """the frame's camera matrix -> row f of the stack's (B,3,3) device buffer (on the current = the submission's stream)"""
        if self._K[j] is None:
            self._K[j] = torch.zeros((self.B, 3, 3), dtype=torch.float32, device=self._stacks[j].img.device)
        if not torch.is_tensor(K):
            K = torch.tensor(K, dtype=torch.float32)
        if tuple(K.shape) != (3, 3):
            raise ValueError("FrameBatcher.submit: K must be a (3,3) camera matrix")
        self._K[j][f].copy_(K, non_blocking=True)

    def _rig_ext(self, j: int):
        """the (ext, rig stride) pair the stack's submission reads in place"""
        dev = self._stacks[j].img.device
        if self.rig_per_rig:
            return self._ext[j], 12 * self.C
        if not self._ext_shared[0].is_cuda:
            self._ext_shared = (self._ext_shared[0].to(dev), 0)
        return self._ext_shared

    def _put_ext(self, j: int, s: int, E):
        """the rig's extrinsics -> entry s of the stack's (S,C,12) device buffer (on the submission's stream), as _put_K fills K"""
        from . import pose as _pose

        dev = self._stacks[j].img.device
        if self._ext[j] is None:
            self._ext[j] = torch.zeros((self.B // self.C, self.C, 12), dtype=torch.float32, device=dev)
        ext, _ = _pose.rig_extrinsics(E, self.C, dev)
        if ext.dim() != 2:
            raise ValueError("FrameBatcher.submit_rig: extrinsics must be the rig's (C,4,4) / (C,3,4)")
        self._ext[j][s].copy_(ext, non_blocking=True)

    def _put_eval(self, j: int, f: int, P_gt, row: int):
        """the frame's ground-truth pose and table row -> entry f of the stack's buffers (on the submission's stream); a stack that starts
        has its rows reset to -1, so the padding frames of a flushed stack write nothing"""
        if self._P[j] is None:
            dev = self._stacks[j].img.device
            self._P[j] = torch.zeros((self.B, 4, 4), dtype=torch.float64, device=dev)   # float64 holds a float32 P_gt exactly
            self._row[j] = torch.full((self.B,), -1, dtype=torch.int32, device=dev)
        if not torch.is_tensor(P_gt):
            P_gt = torch.tensor(P_gt, dtype=torch.float64)
        if tuple(P_gt.shape) != (4, 4):
            raise ValueError("FrameBatcher.submit: P_gt must be a (4,4) pose matrix")
        if f == 0:
            self._row[j].fill_(-1)
        self._P[j][f].copy_(P_gt, non_blocking=True)
        self._row[j][f:f + 1].fill_(int(row))

    def submit(self, pc_data_dict: Dict, img: torch.Tensor, K=None, P_gt=None, row: Optional[int] = None) -> Tuple[int, int, int]:
        """one frame -> a ticket.  The frame's tensors are read by a copy kernel enqueued on the submission's stream before this returns
        control to the caller's NEXT enqueue on that stream only - keep them unmodified until `result()` of any later ticket, or pass
        tensors that are not rewritten (a loader ring).  K: the frame's (3,3) camera matrix (host or device), required with pose=True.
        P_gt, row: the frame's (4,4) ground-truth pose (host or device) and its row of the evaluation table, required with eval_table."""
        if self.C != 1:
            raise ValueError("FrameBatcher(cameras=%d): submit() takes a (cloud, image) pair; a rig goes through submit_rig()" % self.C)
        if self.pose and K is None:
            raise ValueError("FrameBatcher(pose=True): submit() needs the frame's camera matrix K")
        if self.eval_table is not None and (P_gt is None or row is None or int(row) < 0):
            raise ValueError("FrameBatcher(eval_table=...): submit() needs the frame's ground-truth pose P_gt and its table row >= 0")
        j = self._cur
        if self._fill == 0:
            self._collect(j)                      # the stack's previous submission must have been read out before it is overwritten
            self._serial[j] += 1
        cur = torch.cuda.current_stream(img.device)
        s = self._stream(j)
        s.wait_stream(cur)                        # the frame may have been produced on the caller's stream
        with torch.cuda.stream(s):
            # conversions (int64 tables -> int32, non-contiguous inputs -> copies) run ON the submission's stream: their temporaries are
            # blocks of that stream's allocator pool, reused only behind the copy kernel that reads them.  (Made on the caller's stream
            # they could be handed to the NEXT frame's conversions while this stream, queued behind an earlier stack's forward, had not
            # copied them yet.)
            pyr = {k: ([CoFiI2P._as_idx32(t) for t in pc_data_dict[k]] if k != "points" else [p.contiguous() for p in pc_data_dict[k]])
                   for k in FrameStack.KEYS}
            feats = pc_data_dict["feats"].contiguous()
            if self._stacks[j] is None:
                self._stacks[j] = FrameStack(pyr, feats, img, self.B)
            self._stacks[j].put(self._fill, pyr, feats, img)
            if self.pose:
                self._put_K(j, self._fill, K)
            if self.eval_table is not None:
                self._put_eval(j, self._fill, P_gt, row)
        self._last = (pyr, feats, img)
        ticket = (j, self._serial[j], self._fill)
        self._fill += 1
        if self._fill == self.B:
            self._launch(j)
            self._cur, self._fill = (j + 1) % self.ring, 0
        return ticket

    def submit_rig(self, pc_data_dict: Dict, imgs: torch.Tensor, K=None, P_gt=None, rows=None, extrinsics=None) -> List[Tuple[int, int, int]]:
        """one cloud and the C = cameras images that look at it -> C tickets, one per image (for `result`, `fine_xy`, `pose_result`).
        imgs (C,3,H,W); K (C,3,3) camera matrices with pose=True; P_gt (C,4,4) ground-truth poses and rows (C table rows >= 0) with
        eval_table; extrinsics (C,4,4) / (C,3,4), camera <- rig, with rig_extrinsics="per_rig".  The tensors are read as those of `submit`
        are."""
        C = self.C
        if not torch.is_tensor(imgs) or imgs.dim() != 4 or imgs.shape[0] != C:
            raise ValueError("FrameBatcher(cameras=%d): submit_rig() needs the rig's images as one (%d,3,H,W) tensor, got %s"
                             % (C, C, tuple(imgs.shape) if torch.is_tensor(imgs) else type(imgs).__name__))
        if self.pose and (K is None or len(K) != C):
            raise ValueError("FrameBatcher(pose=True): submit_rig() needs the images' camera matrices K (%d,3,3)" % C)
        if self.eval_table is not None and (P_gt is None or rows is None or len(P_gt) != C or len(rows) != C or min(int(r) for r in rows) < 0):
            raise ValueError("FrameBatcher(eval_table=...): submit_rig() needs the images' ground-truth poses P_gt (%d,4,4) and %d table rows >= 0" % (C, C))
        if self.rig_per_rig != (extrinsics is not None):
            raise ValueError("FrameBatcher.submit_rig: extrinsics go with rig_extrinsics='per_rig', and only with it")
        j = self._cur
        if self._fill == 0:
            self._collect(j)
            self._serial[j] += 1
        cur = torch.cuda.current_stream(imgs.device)
        s = self._stream(j)
        s.wait_stream(cur)
        with torch.cuda.stream(s):   # conversions on the submission's stream: see submit()
            pyr = {k: ([CoFiI2P._as_idx32(t) for t in pc_data_dict[k]] if k != "points" else [p.contiguous() for p in pc_data_dict[k]])
                   for k in FrameStack.KEYS}
            feats = pc_data_dict["feats"].contiguous()
            imgs = imgs.contiguous()
            if self._stacks[j] is None:
                self._stacks[j] = FrameStack(pyr, feats, imgs[0], self.B, cameras=C)
            self._stacks[j].put_cloud(self._fill // C, pyr, feats)
            self._stacks[j].put_image(self._fill, imgs)
            if self.rig_per_rig:
                self._put_ext(j, self._fill // C, extrinsics)
            for c in range(C):
                f = self._fill + c
                if self.pose:
                    self._put_K(j, f, K[c])
                if self.eval_table is not None:
                    self._put_eval(j, f, P_gt[c], rows[c])
        self._last = (pyr, feats, imgs)
        tickets = [(j, self._serial[j], self._fill + c) for c in range(C)]
        self._fill += C
        if self._fill == self.B:
            self._launch(j)
            self._cur, self._fill = (j + 1) % self.ring, 0
        return tickets

    def flush(self):
        """submit the partly filled stack (padded with copies of its last frame - of its last rig with cameras > 1)"""
        if self._fill == 0:
            return
        j = self._cur
        pyr, feats, img = self._last
        with torch.cuda.stream(self._stream(j)):
            if self.C != 1:   # img: the last rig's (C,3,H,W); its camera matrices sit in the C rows before the first free one
                for f0 in range(self._fill, self.B, self.C):
                    self._stacks[j].put_cloud(f0 // self.C, pyr, feats)
                    self._stacks[j].put_image(f0, img)
                    if self.pose:
                        self._K[j][f0:f0 + self.C].copy_(self._K[j][self._fill - self.C:self._fill])
                    if self.rig_per_rig:
                        self._ext[j][f0 // self.C].copy_(self._ext[j][self._fill // self.C - 1])
            else:
                for f in range(self._fill, self.B):
                    self._stacks[j].put(f, pyr, feats, img)
                    if self.pose:
                        self._K[j][f].copy_(self._K[j][self._fill - 1])
        self._launch(j)
        self._cur, self._fill = (j + 1) % self.ring, 0

    def drain(self):
        """submit what is pending and wait for every submission in flight (their results stay readable as before)"""
        self.flush()
        for j in range(self.ring):
            self._collect(j)

    def reset(self):
        """wait for every submission in flight and drop a partly filled stack (its frames are not submitted)"""
        for j in range(self.ring):
            self._collect(j)
        self._fill = 0

    def result(self, ticket: Tuple[int, int, int]):
        """-> the reference's 8-tuple of the ticket's frame (views of the slot's static outputs; see the module docstring for their lifetime)"""
        j, serial, f = ticket
        if serial != self._serial[j]:
            raise RuntimeError("FrameBatcher: the ticket's stack has been reused (results live for ring - 1 = %d later submissions)" % (self.ring - 1))
        if j == self._cur and self._fill > 0:
            self.flush()
        self._collect(j)
        if self._results[j] is None:
            raise RuntimeError("FrameBatcher: no submission is pending for this ticket")
        r = self._results[j][f]
        if isinstance(r, Exception):
            raise r                               # this frame only: the other tickets of the stack are served
        return r

    def fine_xy(self, ticket: Tuple[int, int, int]) -> torch.Tensor:
        """-> the fine matches (2, n) of the ticket's frame (eval_all.py:99-105; `handle["fine_xy"][f]` of the stack's submission)"""
        self.result(ticket)   # collects the submission; raises for a stale ticket or a frame without matches
        return self._fine[ticket[0]][ticket[2]]

    def sub_xy(self, ticket: Tuple[int, int, int]) -> torch.Tensor:
        """-> the sub-pixel matches (2, n) of the ticket's frame: column and row on the fine map (`handle["out"][f]["sub_xy"][:, :n]` of
        the stack's submission; ops.fine_refine).  Same lifetime as `result(ticket)`."""
        if not self.subpixel:
            raise RuntimeError("FrameBatcher: built without subpixel=True")
        self.result(ticket)   # collects the submission; raises for a stale ticket or a frame without matches
        j, _, f = ticket
        return self._sub[j][f][:, :self._counts[j][f]]

    def pose_result(self, ticket: Tuple[int, int, int]):
        """-> (result (3,) int32 [success, inliers, winning hypothesis], R (3,3), t (3,), inliers (n,) uint8) of the ticket's frame: device
        views of the slot's pose buffers, same lifetime as `result(ticket)`.  A frame with fewer than 4 matches has result[0] == 0 and the
        identity pose (its `result(ticket)` raises); its neighbours in the stack are not affected."""
        if not self.pose:
            raise RuntimeError("FrameBatcher: built without pose=True")
        j, serial, f = ticket
        if serial != self._serial[j]:
            raise RuntimeError("FrameBatcher: the ticket's stack has been reused (results live for ring - 1 = %d later submissions)" % (self.ring - 1))
        if j == self._cur and self._fill > 0:
            self.flush()
        self._collect(j)
        if self._poses[j] is None:
            raise RuntimeError("FrameBatcher: no submission is pending for this ticket")
        p = self._poses[j]
        return p["result"][f], p["R"][f], p["t"][f], p["inliers"][f, :self._counts[j][f]]

    def rig_pose_result(self, ticket: Tuple[int, int, int]):
        """-> (result (3,) int32 [success, inliers over all cameras, winning hypothesis], R (3,3), t (3,)) of the ticket's RIG (rig <- cloud):
        the same for the C tickets of a rig.  Device views of the slot's buffers, same lifetime as `result(ticket)`."""
        if not self.rig:
            raise RuntimeError("FrameBatcher: built without rig_extrinsics")
        self.pose_result(ticket)   # the ticket checks, the flush and the collection
        r = self._rig_poses[ticket[0]]
        s = ticket[2] // self.C
        return r["result"][s], r["R"][s], r["t"][s]

    def covariance_result(self, ticket: Tuple[int, int, int]):
        """-> (cov (6,6), info (6,6), stat (4,) = [ok, rows used, sigma_hat^2, min_pivot]) float64 of the pose of the ticket's image
        (pose.pose_covariance_batch behind the stack's pose tail).  Device views of the slot's buffers, same lifetime as `result(ticket)`."""
        if not self.covariance:
            raise RuntimeError("FrameBatcher: built without covariance=True")
        self.pose_result(ticket)   # the ticket checks, the flush and the collection
        p, f = self._poses[ticket[0]], ticket[2]
        return p["cov"][f], p["info"][f], p["cov_stat"][f]

    def rig_covariance_result(self, ticket: Tuple[int, int, int]):
        """-> (cov (6,6), info (6,6), stat (4,)) of the pose of the ticket's RIG, in the rig's tangent space (pose.pose_covariance_rig): the
        same for the C tickets of a rig.  Same lifetime as `result(ticket)`."""
        if not self.covariance:
            raise RuntimeError("FrameBatcher: built without covariance=True")
        self.rig_pose_result(ticket)   # refuses a batcher without rig_extrinsics
        r, s = self._rig_poses[ticket[0]], ticket[2] // self.C
        return r["cov"][s], r["info"][s], r["cov_stat"][s]

    def fusion_result(self, ticket: Tuple[int, int, int]) -> Dict[str, torch.Tensor]:
        """-> the registered cloud of the ticket's frame: {"depth" (H,W) float32, "index" (H,W) int32, "flags" (N,) uint8, "stats" (4,) int32}
        of its image, "color" (N,3) and "camera" (N,) int32 of its cloud (fusion.FusionBuffers has the meanings).  With cameras = C the
        four per-image entries hold all C images of the ticket's rig - (C,H,W), (C,H,W), (C,N), (C,4) - the same for its C tickets.
        Device views of the stack's buffers, same lifetime as `result(ticket)`."""
        if not self.fuse:
            raise RuntimeError("FrameBatcher: built without fuse=True")
        self.pose_result(ticket)   # the ticket checks, the flush and the collection
        b, f, C = self._fusion[ticket[0]], ticket[2], self.C
        s = f // C
        img = slice(s * C, (s + 1) * C) if C > 1 else f
        return {"depth": b.depth[img], "index": b.index[img], "flags": b.flags[img], "stats": b.stats[img], "color": b.color[s],
                "camera": b.camera[s]}

    @property
    def submissions(self) -> int:
        return self._nsub
