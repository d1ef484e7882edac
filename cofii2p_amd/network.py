"""Drop-in mirror of the reference's `model/network.py` module surface on MI355X.

`CoFiI2P(opt)` has the reference's constructor, `forward` signature, 8-tuple return and state_dict
layout (model/network.py:14-164; 430 tensors, strict-loadable: evaluation/eval_all.py:49), so it
drops into `evaluation/eval_all.py` / `train.py`-style callers under PyTorch-ROCm.  Underneath,
forward enqueues hand-written gfx950 kernels through the C ABI of libcofi_hip.so
(include/cofi_hip.h).  Inference runs the fused kernel sequence (no graph behind the outputs); mode='train' with autograd enabled runs
the differentiable form of the same network (train_forward.py: HIP kernels forward and backward).  There is no CPU path — the module
raises if the HIP library is missing or a tensor is not on the GPU.
"""
import os
import sys
from typing import Dict, NamedTuple, Optional

import numpy as np
import torch
import torch.nn as nn

from . import _lib, image, kpfpn, ops, transformer
from . import pose as _pose
from .spec import D_MODEL, LAYER_KINDS, N_HEAD, N_LAYERS, is_buffer, state_dict_spec

__all__ = ["CoFiI2P", "CoFiI2P_wrapper", "fine_process", "extract_patch", "point2node", "square_distance", "fine_matching",
           "score_thresholds"]


class _Node(nn.Module):
    """Anonymous container: the parameter tree is generated from spec.state_dict_spec()."""


def _attach(root: nn.Module, name: str, shape, dtype: str):
    parts = name.split(".")
    node = root
    for p in parts[:-1]:
        if p not in node._modules:
            node.add_module(p, _Node())
        node = node._modules[p]
    t = torch.zeros(shape, dtype=torch.int64 if dtype == "int64" else torch.float32)
    if is_buffer(name):
        node.register_buffer(parts[-1], t)
    else:
        node.register_parameter(parts[-1], nn.Parameter(t))   # learnable, as in the reference (train.py:163 filters on requires_grad)


def score_thresholds(n: int = 64) -> np.ndarray:
    """network.py:147-151: ``thrs = 0.9`` then ``thrs -= 0.02`` in python floats; the comparison with
    the fp32 score tensor happens in fp32, hence the cast."""
    out, t = [], 0.9
    for _ in range(n):
        out.append(t)
        t -= 0.02
    return np.asarray(out, dtype=np.float64).astype(np.float32)


ALTERNATE_ORDER = True   # odd forward_async slots run the point encoder first (measured 515-518 vs 510 frames/s)
ROUTING = ("ALTERNATE_ORDER",)   # this module's part of the key of every recording (ops.ROUTING)


def routing_state() -> tuple:
    """The current value of every switch that decides which kernels a forward enqueues (the ROUTING tuples of ops, kpfpn, transformer and
    this module), as one hashable tuple: part of the key of every recording (CoFiI2P._graph_forward, train_step.GraphedTrainStep), so
    that a switch flipped inside a process records anew instead of replaying the old launch sequence.  Read afresh on every call (a
    cached value would be as stale as the recordings it guards).  Not in here: the `static const` getenv switches of
    csrc/gemm_planner.h, which are fixed for the life of the process."""
    state = []
    for module in (ops, kpfpn, transformer, sys.modules[__name__]):
        for name in module.ROUTING:
            v = getattr(module, name)
            if callable(v):
                v = v()
            state.append(tuple(sorted(v.items())) if isinstance(v, dict) else v)
    return tuple(state)


def _as_idx32(t: torch.Tensor) -> torch.Tensor:
    return ops.idx_to_int32(t) if t.dtype != torch.int32 else t.contiguous()


class ForwardInputs(NamedTuple):
    """The inputs of one device-side forward, prepared once: contiguous tensors, int32 index tables.  `order` is a list (empty when the
    pyramid has none), `kpt` / `inl` the labels of mode 'train' / 'val' or None."""
    points: list
    neighbors: list
    subsampling: list
    upsampling: list
    order: list
    feats: torch.Tensor
    img: torch.Tensor
    kpt: Optional[torch.Tensor]
    inl: Optional[torch.Tensor]
    sorted_tables: bool

    @classmethod
    def prepare(cls, pc_data_dict, img, labels=(None, None), inputs_stable: bool = False):
        """inputs_stable: the recording reads these very tensors, so nothing may need a copy or a conversion"""
        if inputs_stable:
            for k in ("points", "neighbors", "subsampling", "upsampling"):
                for t in pc_data_dict[k]:
                    if not t.is_contiguous() or (k != "points" and t.dtype != torch.int32):
                        raise _lib.CofiError("inputs_stable=True reads the inputs in place: contiguous tensors and int32 tables only (%s)" % k)
            if not (pc_data_dict["feats"].is_contiguous() and img.is_contiguous()):
                raise _lib.CofiError("inputs_stable=True reads the inputs in place: contiguous feats / img only")
        tabs = [[_as_idx32(t) for t in pc_data_dict[k]] for k in ("neighbors", "subsampling", "upsampling")]
        return cls([p.contiguous() for p in pc_data_dict["points"]], *tabs, list(pc_data_dict.get("order") or []),
                   pc_data_dict["feats"].contiguous(), img.contiguous(), labels[0], labels[1], bool(pc_data_dict.get("sorted_tables")))

    def flat(self) -> list:
        """every tensor of the record (absent labels as None), in field order"""
        return [*self.points, *self.neighbors, *self.subsampling, *self.upsampling, *self.order, self.feats, self.img, self.kpt, self.inl]

    def rebuild(self, flat):
        """a record of this one's structure over the tensors of another flat list (a recording's static buffers)"""
        it = iter(flat)
        lists = [[next(it) for _ in field] for field in self[:5]]
        return ForwardInputs(*lists, *it, self.sorted_tables)


class _Recording(NamedTuple):
    """one entry of CoFiI2P._graphs"""
    graph: "torch.cuda.CUDAGraph"
    inputs: ForwardInputs          # the tensors the graph reads: the caller's own (inputs_stable) or static buffers
    outs: list
    copy: Optional[ops.MultiCopy]  # inputs of a submission -> the static buffers, one launch (None: inputs_stable)


class _Slot:
    """what a forward_async slot owns on one device next to its recordings (a slot is finished before it is reused)"""

    def __init__(self):
        self.count_host = {}   # frames of a submission -> the pinned landing buffer of their match counts
        self.pose = _pose.PoseTail()


_EXTRA_FRAME_STREAMS = {}   # device -> streams handed out by CoFiI2P.frame_streams beyond the capture and the default stream


class CoFiI2P(nn.Module):
    """See module docstring.  ``opt`` needs ``img_H, img_W, img_fine_resolution_scale, norm``
    (data/options.py:17-19,51).  ``norm``: 'gn' (the shipped configuration, the fast path), 'bn' (inference: running statistics, folded
    into the weights) or 'ln' - the three get_norm() variants of model/kpconv/modules.py:51-60.

    ``arithmetic`` (or ``opt.arithmetic``): how the dense contractions (every nn.Linear / nn.Conv2d / KPConv weight product) are
    computed; storage and accumulation are fp32 in all three.
      "f32"     products on the exact fp32 MFMA, bit-equal to an fmaf chain.
      "bf16x6"  each fp32 operand split into THREE bf16 planes (hi + mid + lo = all 24 mantissa bits), six products on the bf16 matrix
                cores: fp32-GRADE - the same error against fp64 as "f32" (what is dropped is below 2^-24 of |a||b|; golden frame 1.9e-6 vs
                2.0e-6, same matches) at ~1.9x its frame rate.  The default of the reference-named shim ``model.network.CoFiI2P`` and of
                the training path.
      "bf16x3"  two planes (hi + lo), three products: ~2^-16 relative error per product, the fastest (outputs within 2e-5 of the
                reference on the golden frame, same matches selected there, but a score within ~1e-5 of the 0.9 threshold or an arg-max
                near-tie may resolve differently).
    None = the process default (``COFI_GEMM``, "bf16x3" when unset).  INTEGRATION.md states the accuracy contract."""

    # distinct (slot, input set) graphs kept for forward_async(inputs_stable=True).  Every captured graph owns a private memory pool with a
    # full frame of intermediates (≈ 0.1 GB for a KITTI frame: the bench's 16 graphs + weights + planes + inputs peak at 2.35 GB, `peak_mem_GB`;
    # the stress configuration ≈ 20 GB): a loader should recycle
    # a RING of input buffers - one graph per (slot, ring entry) - not allocate fresh inputs per frame; past the limit forward_async raises
    MAX_STABLE_GRAPHS = 64
    DEFAULT_ARITHMETIC = None   # None: follow ops.GEMM_MODE (COFI_GEMM); the model.network shim sets "bf16x6"
    # True: forward() replays a hipGraph per input signature WITHOUT being asked (enable_graphs) and hands out CLONES of the graph's static
    # outputs, so nothing about the call changes for an unchanged caller (the model.network shim: 242 vs 173 frames/s for an eval_all.py-shaped
    # loop); enable_graphs(False) switches it off, enable_graphs(True) keeps the zero-copy views
    DEFAULT_GRAPHS = False
    MAX_COPY_GRAPHS = 8         # input signatures (sizes) whose staged-input graphs are kept; the oldest is dropped beyond that

    def __init__(self, opt, init: str = "synthetic", arithmetic: Optional[str] = None, attention: Optional[str] = None):
        super().__init__()
        self.opt = opt
        self.arithmetic = arithmetic if arithmetic is not None else getattr(opt, "arithmetic", self.DEFAULT_ARITHMETIC)
        ops.arithmetic(self.arithmetic)   # validates the name
        # ATTENTION of transformer.py:12: fixed for the life of the instance (so its graph cache holds one kind only); no parameters depend on it
        self.attention = transformer.check_attention(attention if attention is not None else getattr(opt, "attention", "full"))
        self.pc_norm_kind = getattr(opt, "norm", "gn")   # get_norm() of the point encoder: 'gn' (shipped), 'bn' (running statistics), 'ln'
        if self.pc_norm_kind not in ("gn", "bn", "ln"):
            raise ValueError("only support batch normalization, layer normalization and group normalization now!")   # modules.py:60
        self.pe_H = int(opt.img_H / 8)
        self.pe_W = int(opt.img_W / 8)
        self.H_fine_res = int(round(opt.img_H / opt.img_fine_resolution_scale))
        self.W_fine_res = int(round(opt.img_W / opt.img_fine_resolution_scale))
        for name, (shape, dtype) in state_dict_spec(self.pc_norm_kind).items():
            _attach(self, name, shape, dtype)
        if init == "synthetic":
            from .spec import synth_state_dict

            self.load_state_dict({k: torch.from_numpy(v) for k, v in synth_state_dict(norm=self.pc_norm_kind).items()}, strict=True)
        self._packed: Optional[Dict[str, torch.Tensor]] = None
        self._packed_key = None
        self._replayed_steps = 0   # optimisation steps replayed from a hipGraph (train_step.GraphedTrainStep): they do not bump version counters
        self._trained = False   # set by the first differentiable forward: from then on _pack() watches the parameters' version counters
        self.compute_unused_image_maps = os.environ.get("COFI_DEAD_MAPS", "1") != "0"  # layer3/layer4/avg-pool of the ResNet (network.py:87-89): read by nothing
        self._use_graphs = False
        self._auto_graphs = bool(self.DEFAULT_GRAPHS)
        self._graphs = {}    # key (see _graph_forward) -> _Recording
        self._slots = {}     # (slot, device) -> _Slot
        self._capture = None   # the stream recordings are warmed up and captured on (_capture_stream)
        self._grid_cache = {}

        # intra-frame fork/join slots captured by forward_async (bit 0 image branch, 1 residual shortcuts, 2 attention streams,
        # 3 the ResNet tail nothing reads)
        self.async_branch_mask = int(os.environ.get("COFI_ASYNC_BRANCH_MASK", "0"))
        self.register_load_state_dict_post_hook(lambda module, incompatible: module._invalidate())
        self.eval()

    # ------------------------------------------------------------------ weights
    def _drop_recordings(self):
        """every recording, with its static inputs, its outputs and its staging copy; the slots' own buffers (pinned counts, pose tails)
        depend on neither the weights nor a recording and stay"""
        self._graphs = {}

    def _invalidate(self):
        self._packed = None
        self._drop_recordings()

    def _apply(self, fn, *a, **k):
        self._invalidate()
        return super()._apply(fn, *a, **k)

    def _param_versions(self) -> int:
        return sum(t._version for t in self.parameters()) + sum(t._version for t in self.buffers())

    def _pack(self, device) -> Dict[str, torch.Tensor]:
        # the packed (folded, pre-split) weights are a function of the parameters: an optimizer step (in-place update, train.py:286)
        # bumps the tensors' version counters, and the next inference forward (train.py's validation pass) packs again
        # (checked only once the training path has run: the serving loop does not pay for 430 version reads per frame)
        stamp = (device, self._param_versions() + self._replayed_steps if self._trained else 0)
        if self._packed is not None and self._packed_key == stamp:
            return self._packed
        if self._packed is not None:
            self._drop_recordings()
        sd = {k: v.detach() for k, v in self.state_dict().items()}
        for k, v in sd.items():
            if v.device != device:
                raise _lib.CofiError("parameter %s is on %s but the inputs are on %s (call .cuda())" % (k, v.device, device))
        P: Dict[str, torch.Tensor] = {}
        P.update(kpfpn.pack_encoder(sd))
        P.update(image.pack_image(sd))
        for k, v in sd.items():
            if k.startswith("pc_feature_layer."):
                P[k] = v.contiguous()
        for head in ("pc_score_layer", "img_score_layer"):
            for i in (0, 3, 6):
                w = sd["%s.%d.weight" % (head, i)]
                P["%s.%d.weight" % (head, i)] = w.reshape(w.shape[0], w.shape[1]).contiguous()
        # the last score GEMM has K = 64 -> fine (K % 4 == 0)
        self._layers = [transformer.pack_layer(sd, "transformer.layers.%d." % l) for l in range(N_LAYERS)]

        def gemm_weight(k, v):  # every static GEMM operand: (N, K) fp32 matrices used as `w` of ops.gemm* / conv2d_nhwc
            return (torch.is_tensor(v) and v.dim() == 2 and v.dtype == torch.float32 and v.shape[1] % 4 == 0
                    and k.endswith(("weight", "weights", ".nhwc")))

        for d in [P] + self._layers:   # split once into bf16 hi/lo planes (the bf16x3 kernels read those; fp32 mode reads .w)
            for k in list(d):
                # (the unsplit weight of a decoder that always runs in the projected form is not read; the concat form splits on first use)
                if gemm_weight(k, d[k]) and not kpfpn.decoder_weight_unused(k):
                    d[k] = ops.presplit(d[k])
        self._packed, self._packed_key = P, stamp
        return P

    # ------------------------------------------------------------------ forward pieces
    def _pixel_grid(self, H8: int, W8: int, B: int, dev) -> torch.Tensor:
        key = (H8, W8, B, str(dev))
        g = self._grid_cache.get(key)
        if g is None:
            gy, gx = torch.meshgrid(torch.arange(H8, device=dev, dtype=torch.int32), torch.arange(W8, device=dev, dtype=torch.int32),
                                    indexing="ij")
            g = self._grid_cache[key] = torch.stack([gy, gx], -1).reshape(H8 * W8, 2).repeat(B, 1).contiguous()
        return g

    _as_idx32 = staticmethod(_as_idx32)

    def _score_head(self, P, head: str, tokens: torch.Tensor, frames: int = 1) -> torch.Tensor:
        """network.py:42-43 on token-major data: 1x1 conv = GEMM, InstanceNorm over positions = per-column
        normalisation (group width 1), ReLU = slope 0; each InstanceNorm + ReLU is applied by the operand loader of the
        next GEMM (ops.Normed), falling back to the stand-alone kernels where the 64-row statistics slabs straddle frames."""
        T = tokens.shape[0]

        def in_relu(y, part):
            if frames > 1 and (T // frames) % 64:   # slabs straddle frames: statistics by a separate pass over the rows
                return ops.group_norm_apply(y, ops.group_stats(y, y.shape[1], frames=frames), slope=0.0, frames=frames)
            return ops.Normed(y, ops.ColStats(part, T, y.shape[1], frames), slope=0.0)

        y, part = ops.gemm_colstats(tokens, P[head + ".0.weight"])
        y, part = ops.gemm_colstats(in_relu(y, part), P[head + ".3.weight"], frames=frames)
        return ops.gemm(in_relu(y, part), P[head + ".6.weight"], act=ops.ACT_SIGMOID, frames=frames)  # (T,1)

    def _pc_feature_mlp(self, P, x: torch.Tensor, out=None, l2norm: bool = False) -> torch.Tensor:
        """network.py:29; l2norm: followed by F.normalize(dim=1) (network.py:84) in the last GEMM's epilogue."""
        p = "pc_feature_layer."
        y = ops.layer_norm(ops.gemm(x, P[p + "0.weight"]), P[p + "1.weight"], P[p + "1.bias"], relu=True)
        y = ops.layer_norm(ops.gemm(y, P[p + "3.weight"]), P[p + "4.weight"], P[p + "4.bias"], relu=True)
        return ops.gemm(y, P[p + "6.weight"], out=out, l2norm=l2norm)

    # ------------------------------------------------------------------ device-side forward (no host sync)
    def _run_device(self, P, points, neighbors, subsampling, upsampling, feats, img, mode, fine_center_kpt_coors,
                    fine_pc_inline_index, taps=None, order=None, pc_first: bool = False, cameras: int = 1, sorted_tables: bool = False,
                    subpixel: bool = False):
        """Everything of network.py:74-161 that runs on the device.  Test-mode outputs are sized at
        capacity (N4 rows) with the match count left in device memory: capturable in a hipGraph.

        STACK MODE: ``img`` is (B,3,H,W) and every point-side tensor holds B equally sized frames stacked along
        its rows (index tables frame-local).  All per-frame statistics (GroupNorm, InstanceNorm, the token-axis
        Q normalisation), the neighbour gathers, attention and the matching are computed per frame inside the
        same launches; row-wise kernels (GEMMs, LayerNorm, ...) just see B times more rows.  Outputs are lists
        with one entry per frame.

        RIG (cameras = C > 1, mode='test'): the B images are those of S = B // C clouds, image f looking at cloud f // C.  The point-side
        tensors hold S frames; the KPConv-FPN, the point MLP and the position encoding run once per cloud and the coarse point tokens are
        copied C times into the transformer's point stream (ops.repeat_frames).  From there on everything is per image, as in stack
        mode; the matching tail reads the points and fine descriptors of cloud f // C.  Outputs: B per-image records, laid out as a
        stack-mode submission of B frames lays them out.

        subpixel (mode='test'): the sub-pixel refinement of the fine matches (ops.fine_refine: one launch for all B frames right behind
        match_finish, while the fine map is live) - per-frame "sub_xy" (2, cap) and "sub_peak" (cap,), outs[0]["sub_xy_all"] (B, 2, cap)
        and outs[0]["fine_img_map"], the map it read."""
        dev = img.device
        if subpixel and mode != "test":
            raise ValueError("subpixel=True refines the fine matches of mode='test'; mode=%r has none" % (mode,))
        B = img.shape[0]
        if cameras != 1 and (mode != "test" or taps is not None):
            raise ValueError("a rig (cameras = %d > 1) serves mode='test' only (forward_async): mode=%r shares no cloud between images" % (cameras, mode))
        if cameras < 1 or B % cameras:
            raise _lib.CofiError("cameras = %d does not divide the B = %d images of the submission" % (cameras, B))
        S = B // cameras   # clouds
        if mode not in ("test", "val") and B != 1:
            raise ValueError("stack mode (B > 1) serves mode='test' and mode='val'")
        # mode='val' with labels of a whole submission - fine_center_kpt_coors (B, 2, K), fine_pc_inline_index (B, K), int64 / int32 device
        # tensors - takes the batched label gathers (forward_val_async); the (2, K) / (K,) labels of forward() keep the single-frame launches
        val_batched = mode == "val" and fine_center_kpt_coors is not None and fine_center_kpt_coors.dim() == 3
        if B != 1 and mode == "val" and not val_batched:
            raise ValueError("stack mode (B > 1) in mode='val' needs labels of shape (B, 2, K) / (B, K): forward_val_async")
        N4 = points[-1].shape[0] // S   # per cloud
        H8, W8 = img.shape[2] // 8, img.shape[3] // 8
        T_img, C = H8 * W8, D_MODEL
        ts = transformer.TokenStreams(B * T_img, B * N4, D_MODEL, dev)
        # ---- image branch (network.py:77,90,104-106,110) on a side stream, concurrent with the point encoder
        br_dead = ops.Branch(dev, 3)  # ResNet layer3/layer4/avg-pool: computed (reference parity), read by nothing downstream

        def image_branch():
            with ops.Branch(dev, 0) as br:
                grid = self._pixel_grid(H8, W8, B, dev)   # (y, x) of every token of the 1/8 map: a constant, built once
                img_set, dims = image.resnet34_nhwc(P, img, full=self.compute_unused_image_maps, tail_branch=br_dead)
                s2_, s4_, s8_ = img_set[0], img_set[1], img_set[2]  # (B*H*W, C) pixel-major
                # the normalised s8 map feeds the transformer AND the up-sampler (network.py:90,129): one launch, two destinations
                s8n_ = torch.empty_like(s8_)
                ops.l2norm_rows2(s8_, s8n_, ts.img[0][:, :D_MODEL])
                ops.pos_sine(grid, ts.img[0], accumulate=True)
            return br, s2_, s4_, s8n_

        def point_branch():   # network.py:76,83-84,107,111
            # F.normalize of the fine point descriptors (network.py:83) rides in decoder2's GEMM epilogue (taps: the raw decoder output is wanted)
            pc_set_ = kpfpn.run_fpn(P, points, neighbors, subsampling, upsampling, feats, taps=taps, frames=S, order=order, l2norm_fine=taps is None,
                                    sorted_tables=sorted_tables)
            fine_pc_ = pc_set_[0] if taps is None else ops.l2norm_rows(pc_set_[0])  # (S*N1,64)
            # a rig: the tokens of the S clouds are made once, then copied in front of each of the cloud's cameras
            tok = ts.pc[0] if cameras == 1 else torch.empty((S * N4, D_MODEL), dtype=torch.float32, device=dev)
            self._pc_feature_mlp(P, pc_set_[-1], out=tok[:, :D_MODEL], l2norm=True)   # ... and of the coarse tokens (network.py:84) in the MLP's last GEMM
            ops.pos_sine(points[-1], tok, accumulate=True)
            if cameras != 1:
                ops.repeat_frames(tok, ts.pc[0][:, :D_MODEL], S, cameras)
            return pc_set_, fine_pc_

        # The two encoders are independent.  In a LINEAR capture (forward_async) their order is free: odd slots run the point encoder
        # first, so that frames in flight on different streams do not march through the same kernels in lock step (complementary
        # kernels - full-grid gathers next to small-grid convolutions - overlap better than two copies of the same one).
        if pc_first:
            pc_set, fine_pc = point_branch()
            br_img, s2, s4, s8n = image_branch()
        else:
            br_img, s2, s4, s8n = image_branch()
            pc_set, fine_pc = point_branch()
        br_img.join(s2, s4, s8n, ts.img[0])
        if taps is not None:
            taps["tok_img"], taps["tok_pc"] = ts.img_tokens().clone(), ts.pc_tokens().clone()

        # ---- fine image descriptors (network.py:129-130): only image data -> side stream, under the transformer
        with ops.Branch(dev, 0) as br_up:
            up4 = image.upsample_stage_nhwc(P, "img_upsample_1", s8n, H8, W8, s4, frames=B)
            up2 = image.upsample_stage_nhwc(P, "img_upsample_2", up4, 2 * H8, 2 * W8, s2, frames=B, l2norm=True)  # (B*H2*W2, C2) pixel-major fine image descriptors
            H2, W2, C2 = 4 * H8, 4 * W8, up2.shape[1]

        # ---- transformer (network.py:113-115)
        # the descriptors' L2 normalisation (network.py:125-126) and, for a single frame, their channel-major output layout are written
        # by the last layer's tails when the fused chain runs (transformer._run_chain)
        pc_desc_tok = torch.empty((B * N4, C), dtype=torch.float32, device=dev)   # token-major copies for the similarity GEMM
        img_desc_tok = torch.empty((B * T_img, C), dtype=torch.float32, device=dev)
        img_desc_t = torch.empty((C, T_img), dtype=torch.float32, device=dev) if B == 1 else None
        pc_desc_t = torch.empty((C, N4), dtype=torch.float32, device=dev) if B == 1 else None
        tok_img, tok_pc, l2_done = transformer.run_transformer(self._layers, LAYER_KINDS, ts, N_HEAD, frames=B,
                                                               l2=(img_desc_tok, pc_desc_tok, img_desc_t, pc_desc_t), attention=self.attention)

        # ---- scores + coarse descriptors (network.py:123-126)
        pc_score = self._score_head(P, "pc_score_layer", tok_pc, B)  # (B*N4,1)
        img_score = self._score_head(P, "img_score_layer", tok_img, B)  # (B*T,1)
        if not l2_done:
            ops.l2norm_rows(tok_pc, out=pc_desc_tok)
            ops.l2norm_rows(tok_img, out=img_desc_tok)
            img_desc_t = pc_desc_t = None
        br_up.join(up2)
        if taps is not None:
            taps.update(up2=up2, fine_pc=fine_pc, tok_img_out=tok_img, tok_pc_out=tok_pc)
        N1 = points[1].shape[0] // S   # per cloud
        P2 = H2 * W2
        # ---- per-frame output layouts + matching: one launch each for all B frames (network.py:145-161; the count stays on the device)
        if img_desc_t is None:   # B > 1 (or no fused chain): channel-major descriptor outputs of every frame
            img_t, pc_t = ops.transpose(img_desc_tok, frames=B).reshape(B, C, T_img), ops.transpose(pc_desc_tok, frames=B).reshape(B, C, N4)
        else:
            img_t, pc_t = img_desc_t[None], pc_desc_t[None]
        test = mode not in ("train", "val")
        if test:
            sim = torch.empty((B * N4, T_img), dtype=torch.float32, device=dev)
            for f in range(B):   # <pc, pixel> per frame (the only per-frame launches left)
                ops.gemm(pc_desc_tok[f * N4:(f + 1) * N4], img_desc_tok[f * T_img:(f + 1) * T_img], out=sim[f * N4:(f + 1) * N4])
            pix = ops.row_argmin_1m(sim)
            sel, xy, cnt = ops.select_matches(pc_score.reshape(-1), pix, W8, H8, score_thresholds(), 4, frames=B)
            sel, xy, cnt = sel.reshape(B, N4), xy.reshape(B, 2, N4), cnt.reshape(B, 2)
            if C2 <= 128:   # coarse point, point2node, patch, fine descriptor and the caller's fine matching (eval_all.py:99-105): one launch
                cpts, pat, fpcs, fxy, fbest = (t if B > 1 else t[None] for t in
                                               ops.match_finish(points[-1], points[1], sel, cnt, up2, H2, W2, xy, fine_pc, 4.0, frames=B, cameras=cameras))
                if subpixel:   # every operand is per image: a rig needs nothing special
                    sxy, spk = (t if B > 1 else t[None] for t in ops.fine_refine(up2, H2, W2, xy, fpcs, fbest, cnt, 4.0, frames=B))
        if val_batched:   # network.py:137-141 for all frames: one launch (cofi_val_gather), labels read in place
            K = fine_center_kpt_coors.shape[2]
            if tuple(fine_center_kpt_coors.shape) != (B, 2, K) or tuple(fine_pc_inline_index.shape) != (B, K):
                raise _lib.CofiError("mode='val' stack labels: fine_center_kpt_coors (B, 2, K) and fine_pc_inline_index (B, K) with B = %d" % B)
            pat_all, fpc_all = ops.val_gather(up2, H2, W2, fine_pc, fine_center_kpt_coors, fine_pc_inline_index)
        outs = []
        for f in range(B):  # per-frame views
            o = {"img_desc": img_t[f].reshape(1, C, H8, W8), "pc_desc": pc_t[f],
                 "img_score": img_score[f * T_img:(f + 1) * T_img].reshape(1, 1, H8, W8), "pc_score": pc_score[f * N4:(f + 1) * N4].reshape(1, 1, N4)}
            cl = f // cameras   # the frame's cloud
            fpc = fine_pc[cl * N1:(cl + 1) * N1]
            up2_f = up2[f * P2:(f + 1) * P2]
            if val_batched:
                o["patches"], o["fine_pc"] = pat_all[f].reshape(K, C2, 4, 4), fpc_all[f]
            elif not test:
                K = fine_center_kpt_coors.shape[1]
                cntk = torch.zeros((2,), dtype=torch.int32, device=dev)
                cntk[:1].fill_(K)   # a fill kernel, not a host-to-device copy: capturable in a hipGraph
                ctr = fine_center_kpt_coors.to(torch.float32).contiguous()
                pat_k = ops.extract_patches_nhwc(up2_f, H2, W2, ctr, cntk, K, 1.0)
                o["patches"] = pat_k.reshape(K, C2, 4, 4)
                o["fine_pc"] = ops.gather_rows(fpc, self._as_idx32(fine_pc_inline_index.reshape(-1)))
            else:
                if C2 <= 128:
                    o["coarse_pts"], o["patches"], o["fine_pc"], o["fine_xy"], o["fine_best"] = cpts[f], pat[f], fpcs[f], fxy[f], fbest[f]
                    if subpixel:
                        o["sub_xy"], o["sub_peak"] = sxy[f], spk[f]
                else:
                    pts4, pts1 = points[-1][cl * N4:(cl + 1) * N4], points[1][cl * N1:(cl + 1) * N1]
                    o["coarse_pts"] = ops.gather_points_sel(pts4, sel[f], cnt[f])
                    node = ops.nearest_node_sel(pts1, pts4, sel[f], cnt[f])
                    o["patches"] = ops.extract_patches_nhwc(up2_f, H2, W2, xy[f], cnt[f], N4, 4.0)
                    o["fine_pc"] = ops.gather_rows_sel(fpc, node, cnt[f], N4)
                    o["fine_xy"], o["fine_best"] = ops.fine_match(o["patches"], o["fine_pc"], xy[f], cnt[f], 4.0)  # eval_all.py:99-105
                    if subpixel:
                        o["sub_xy"], o["sub_peak"] = ops.fine_refine(up2_f, H2, W2, xy[f], o["fine_pc"], o["fine_best"], cnt[f], 4.0)
                o.update(sel=sel[f], coarse_xy=xy[f], count=cnt[f])
            outs.append(o)
        if test:
            outs[0]["count_all"] = cnt   # (B, 2): one device-to-host copy serves every frame of the submission
            if C2 <= 128:   # what a batched consumer of the matches reads in place (pose.solve_pnp_ransac_batch): (B, cap, 3), (B, 2, cap)
                outs[0]["coarse_pts_all"], outs[0]["fine_xy_all"] = cpts, fxy
                if subpixel:   # ... and what it reads instead of fine_xy_all (pose.image_points)
                    outs[0]["sub_xy_all"] = sxy
            if subpixel:   # the map the refinement read stays with the submission: (B * H2 * W2, C2) pixel-major, its second operand
                outs[0]["fine_img_map"] = up2
        if val_batched:   # what the batched consumer (validation.val_monitors) reads in place, and the maps the gathers came from
            outs[0].update(patches_all=pat_all, fine_pc_all=fpc_all, img_desc_all=img_t, pc_desc_all=pc_t, pc_score_all=pc_score,
                           points4=points[-1], fine_img_map=up2, fine_pc_map=fine_pc)
        br_dead.join()
        return outs

    # ------------------------------------------------------------------ hipGraph replay
    def enable_graphs(self, flag: bool = True):
        """Capture the device-side forward in a hipGraph per input signature and replay it: ~450 kernel
        launches per frame become one graph launch (the eager path is CPU-launch bound at batch 1).
        Inputs are staged into static buffers; returned tensors are views of static outputs that the NEXT
        forward overwrites (clone them to keep them)."""
        self._use_graphs = bool(flag)
        if not flag:
            self._auto_graphs = False
            self._drop_recordings()
        return self

    def _capture_stream(self, dev) -> "torch.cuda.Stream":
        """the capture stream of this device: recordings are warmed up AND captured on it, frame_streams hands it out first"""
        if self._capture is None or self._capture.device != dev:
            self._capture = torch.cuda.Stream(device=dev)
        return self._capture

    def _graph_forward(self, P, inputs: ForwardInputs, mode, slot: int = 0, branch_mask: int = 7, inputs_stable: bool = False,
                       cameras: int = 1, subpixel: bool = False):
        def sig(t):
            if t is None:
                return None
            if inputs_stable:   # the graph reads the caller's tensors in place: their addresses are part of its identity
                if not t.is_contiguous():
                    raise _lib.CofiError("inputs_stable=True needs contiguous input tensors")
                return (tuple(t.shape), str(t.dtype), t.data_ptr())
            return (tuple(t.shape), str(t.dtype))

        tensors, dev = inputs.flat(), inputs.img.device
        # what the call itself fixes of the launch sequence, then every switch (routing_state), then the tensor signatures
        key = ("stable" if inputs_stable else "copy", mode, str(dev), slot, branch_mask, cameras, inputs.sorted_tables,
               self.compute_unused_image_maps) + routing_state() + tuple(sig(t) for t in tensors)
        if subpixel:   # one launch more in the recording; the key of every other submission stays what it was
            key += ("subpixel",)
        with ops.recording_scope(slot, branch_mask):   # the slot's scratch namespace; which intra-frame forks the capture records
            rec = self._graphs.get(key)
            if rec is None:
                if inputs_stable:
                    if sum(1 for k_ in self._graphs if k_[0] == "stable") >= self.MAX_STABLE_GRAPHS:
                        raise _lib.CofiError("inputs_stable=True: more than %d distinct input sets; recycle the input buffers or pass "
                                             "inputs_stable=False" % self.MAX_STABLE_GRAPHS)
                    static = inputs   # the entry keeps the tensors alive for as long as the graph exists
                else:
                    copies = [k_ for k_ in self._graphs if k_[0] == "copy"]
                    if len(copies) >= self.MAX_COPY_GRAPHS:   # a caller whose frames keep changing size: bounded memory, oldest signature first
                        del self._graphs[copies[0]]
                    static = inputs.rebuild([None if t is None else torch.empty_like(t).copy_(t) for t in tensors])

                def run():
                    return self._run_device(P, static.points, static.neighbors, static.subsampling, static.upsampling, static.feats, static.img,
                                            mode, static.kpt, static.inl, taps=None, order=static.order or None,
                                            pc_first=ALTERNATE_ORDER and branch_mask == 0 and bool(slot & 1), cameras=cameras,
                                            sorted_tables=static.sorted_tables, subpixel=subpixel)

                # warm-up AND capture run on one persistent stream, so every per-stream workspace is grown (in the
                # ordinary allocator pool) before the capture starts and nothing is allocated for it inside
                cap = self._capture_stream(dev)
                cap.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(cap):
                    for _ in range(2):
                        run()
                torch.cuda.current_stream().wait_stream(cap)
                torch.cuda.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph, stream=cap):
                    outs = run()
                rec = self._graphs[key] = _Recording(graph, static, outs, None if inputs_stable else ops.MultiCopy(dev))
            if rec.copy is not None:
                # per-frame inputs -> the static buffers the graph reads: one batched copy launch (20+ tensors)
                rec.copy.run([None if t is None else t.contiguous() for t in tensors], rec.inputs.flat())
            rec.graph.replay()
        return rec.outs

    # ------------------------------------------------------------------ frames in flight / stack-mode batches
    @staticmethod
    def stack_frames(pyramids, imgs):
        """B single-frame inputs -> one stack-mode input: every tensor concatenated along its rows (index tables stay
        frame-local, int32), images stacked to (B,3,H,W).  All frames must have identical sizes.  The two lists need not be equally
        long: S pyramids and B = S * C images (the C images of cloud 0 first, then those of cloud 1, ...) are the input of a rig
        submission, `forward_async(slot, stacked, imgs, cameras=C)`."""
        out = {}
        for k in ("points", "neighbors", "subsampling", "upsampling"):
            out[k] = [torch.cat([CoFiI2P._as_idx32(p[k][i]) if k != "points" else p[k][i] for p in pyramids], 0).contiguous()
                      for i in range(len(pyramids[0][k]))]
        out["feats"] = torch.cat([p["feats"] for p in pyramids], 0).contiguous()
        if all("order" in p for p in pyramids):
            out["order"] = [torch.cat([p["order"][i] for p in pyramids], 0).contiguous() for i in range(len(pyramids[0]["order"]))]
        if all(p.get("sorted_tables") for p in pyramids):   # the promise of sorted neighbour rows holds for the stack only if every frame gives it
            out["sorted_tables"] = True
        return out, torch.cat([im.reshape(1, *im.shape[-3:]) for im in imgs], 0).contiguous()

    def frame_streams(self, n: int, device=None):
        """The HIP streams to keep n frames in flight on (one `forward_async` slot - or two, alternating - per stream).
        HIP multiplexes all streams of a process onto GPU_MAX_HW_QUEUES (default 4) hardware queues, and the command processor serves
        them best one queue per frame stream: four frame streams run 575-585 frames/s, five 341, six 379 (two then share a queue), and
        raising GPU_MAX_HW_QUEUES does not help (8 queues / 8 streams: 462).  The streams handed out are the ones the process already
        owns - the graph-capture stream and the device's default stream - before new ones are created.  With the default queue
        configuration this is a convenience, not a requirement: four FRESH streams, or a fifth stream that a loader / RCCL uses next to
        the four, run at the same rate (profiles/r03_fifth_stream.md; the round-2 pipeline lost 45 % there)."""
        dev = torch.device(device) if device is not None else next(self.parameters()).device
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())   # 'cuda' and 'cuda:0' are one pool
        pool = [self._capture_stream(dev), torch.cuda.default_stream(dev)]
        # the extra streams are created once per device and process: HIP binds a stream to the least-loaded hardware queue when it is
        # created, so fresh streams per call would land on different queues from one call to the next (a pipeline with the KNN pyramid in
        # the chain measured 355 or 478 frames/s depending on that)
        extra = _EXTRA_FRAME_STREAMS.setdefault(str(dev), [])
        while len(extra) < n - len(pool):
            extra.append(torch.cuda.Stream(device=dev))
        return (pool + extra)[:n]

    @torch.no_grad()
    def forward_async(self, slot: int, pc_data_dict, img, mode: str = "test", inputs_stable: bool = False, pose_K=None,
                      pose_iterations: int = 10000, pose_seed: int = 0, eval_into=None, cameras: int = 1, rig_extrinsics=None, fuse_into=None,
                      pose_cov=False, subpixel: bool = False):
        """Enqueue one test-mode forward on the CURRENT stream through the hipGraph of slot `slot` and return
        immediately (no host sync).  `img` (1,3,H,W) = one frame, or (B,3,H,W) with a stack-mode `pc_data_dict`
        (see stack_frames) = B frames through the same launches.  Slots own their static buffers and scratch, so
        several submissions can be in flight on different streams; `finish(handle)` synchronises on that
        submission only.  A slot must be finished before it is reused.

        inputs_stable=False: the inputs are copied into the slot's static buffers first (one batched launch, 27 MB for a KITTI frame),
        so any tensors may be passed.  inputs_stable=True: the caller promises that these very tensors (contiguous, device-resident,
        int32 tables) stay allocated and unmodified until `finish()`; the graph then reads them IN PLACE - no staging copy - and is
        cached per (slot, input addresses): the natural mode for a loader that recycles a ring of input buffers
        (at most MAX_STABLE_GRAPHS distinct sets).

        pose_K (camera matrices, (B,3,3) or one (3,3) for all frames; host or device): the pose of every frame is solved behind the
        forward on the same stream (pose.solve_pnp_ransac_batch reading the submission's coarse points, coordinate-major fine_xy and
        device-side counts in place; frame f uses seed pose_seed + f) and the handle gains handle["pose"] = {"result" (B,3) int32,
        "R" (B,3,3), "t" (B,3), "inliers" (B,cap) uint8}: device tensors owned by the slot, valid like the other outputs until the slot
        is reused, and complete when `finish(handle)` returns.  A float32 device (B,3,3) pose_K is read in place (keep it unmodified
        until `finish()`); anything else is copied into a buffer of the slot.

        eval_into=(table, P_gt, row_index) (needs pose_K): the evaluation monitors of every frame (evaluation.eval_monitors, one launch)
        are enqueued behind the pose tail, before the handle's `done` event: frame f writes row row_index[f] of `table`
        (evaluation.EvalTable), a negative index nothing.  P_gt (B,4,4) float64 or float32 and row_index (B,) int32 are contiguous device
        tensors read in place (keep them unmodified until `finish()`).  With the default None nothing about the call, its handle or its
        captured graphs changes.

        cameras = C > 1: a RIG submission - the B images are those of S = B // C clouds, C consecutive images per cloud (image f looks at
        cloud f // C: six cameras around one sweep, a stereo pair, several images against one sub-map).  `pc_data_dict` holds the S
        clouds in stack-mode layout (`stack_frames(S pyramids, B images)` builds exactly this input; preprocess.FrameStack(cameras=C)
        fills it in place), and the point encoder runs once per cloud instead of once per image.  Outputs, handle, pose tail (pose_K
        (B,3,3)) and eval_into are those of a stack-mode submission of B frames.  Refused before anything is enqueued: a C that does not
        divide B, point-side rows that S does not divide.

        rig_extrinsics (needs cameras = C > 1 and pose_K): the C cameras are bolted to one body, and the pose tail becomes ONE solve per
        rig over the matches of all its cameras (pose.solve_pnp_ransac_rig; rig s uses seed pose_seed + s).  (C,4,4) / (C,3,4) shared by
        all rigs or (S,C,4,4) / (S,C,3,4), camera <- rig (Y_cam = R_c Y_rig + t_c), a host array (checked, copied into a buffer of the
        slot) or the pair pose.rig_extrinsics returned (read in place: keep it unmodified until `finish()`).  handle["pose"] keeps its
        four per-image entries - now E_c o rig pose, this image's inliers of the rig's consensus, its mask - so eval_into and every other
        reader of per-image poses work unchanged, and the handle gains handle["rig_pose"] = {"result" (S,3) int32 [success, inliers over
        all cameras, hypothesis], "R" (S,3,3), "t" (S,3)}.  Refused before anything is enqueued: rig_extrinsics without pose_K or with
        cameras == 1.

        fuse_into=buffers (a fusion.FusionBuffers; needs pose_K): the registered cloud of the submission (fusion.fuse_into: depth and
        point-id maps per image, in-picture / visible flags, one colour and camera per point) is enqueued behind the pose tail - the rig
        pose tail with rig_extrinsics - on the same stream, before the handle's `done` event.  It reads the submission's finest points
        (`points[0]`: S = B // cameras clouds of N rows), its images, the per-image poses and results of handle["pose"], and pose_K with
        k_scale = image width / fine-map width (pose_K belongs to the fine map the matches live on).  handle["fusion"] = buffers.  Refused
        before anything is enqueued: fuse_into without pose_K, buffers that were not made for (S, N, B, H, W, 3) on the device of the
        images.  With the default None nothing about the call, its handle or its launches changes.

        pose_cov=True, or the 1-sigma pixel noise as a number (needs pose_K): the 6 x 6 covariance of every pose (pose.pose_covariance_batch:
        one launch behind the pose tail, on the same stream, before the handle's `done` event).  handle["pose"] gains "cov" (B,6,6), "info"
        (B,6,6) and "cov_stat" (B,4) float64, owned by the slot like the poses.  With rig_extrinsics handle["rig_pose"] gains the same three
        entries, (S, ...), from pose.pose_covariance_rig in the rig's tangent space, and the per-image entries are the frame form at E_c o rig
        pose on that image's own rows.  True estimates the pixel variance from the residuals.  Refused before anything is enqueued:
        pose_cov without pose_K, a pixel noise that is not a finite number > 0.  With the default False nothing about the call, its handle,
        its buffers or its launches changes.

        subpixel=True: sub-pixel fine matches (ops.fine_refine, INTEGRATION.md "Sub-pixel matches": one launch for all frames inside the
        recorded forward, right behind match_finish).  handle["out"][f] gains "sub_xy" (2, cap) - column and row on the fine map of the
        matched cell, decoded geometrically (best % 4, best // 4; fine_xy keeps the reference caller's transposed decode), plus a parabolic
        offset in [-0.5, 0.5] per axis - and "sub_peak" (cap,), handle["out"][0] gains "sub_xy_all" (B, 2, cap) and "fine_img_map", the
        (B * H2 * W2, C2) pixel-major fine image map the refinement read; rows at or beyond a frame's count are undefined.  Every reader of
        the submission's image points (pose.image_points: the pose tail of frames and rigs, the covariance, eval_into, and fuse_into
        through the poses) then works from sub_xy_all.  fine_xy, fine_best and what finish() returns stay bit for bit what they are.
        Part of the recording's key.  Refused before anything is enqueued: any mode but 'test'.  With the default False nothing about the
        call, its recordings, its handle or its launches changes."""
        B = img.shape[0] if img.dim() == 4 else 1
        subpixel = bool(subpixel)
        if subpixel and mode != "test":
            raise ValueError("forward_async(subpixel=True) refines the fine matches of mode='test', got mode=%r" % (mode,))
        if pose_cov is not False and pose_cov is not None:
            if pose_K is None:
                raise _lib.CofiError("forward_async(pose_cov=...): the covariance belongs to the pose tail - pass pose_K")
            pose_cov = (_pose._sigma(pose_cov) or None,)   # (None,): estimate the pixel variance
        else:
            pose_cov = None
        if mode != "test":
            if cameras != 1:
                raise ValueError("a rig (cameras = %d > 1) serves mode='test' only, got mode=%r" % (cameras, mode))
            raise ValueError("forward_async serves the test-mode pipeline")
        _lib.load()
        S = self._check_rig(pc_data_dict, B, cameras)
        if rig_extrinsics is not None:
            if pose_K is None:
                raise _lib.CofiError("forward_async(rig_extrinsics=...): the rig pose is a pose tail - pass pose_K")
            if cameras == 1:
                raise _lib.CofiError("forward_async(rig_extrinsics=...): a rig has cameras > 1; one camera is served by pose_K alone")
            if not isinstance(rig_extrinsics, tuple):   # checked (and converted) before anything is enqueued
                rig_extrinsics = _pose.rig_extrinsics(rig_extrinsics, cameras, "cpu")
            ext = rig_extrinsics[0]
            if not (torch.is_tensor(ext) and tuple(ext.shape) in ((cameras, 12), (S, cameras, 12))):
                raise _lib.CofiError("forward_async(rig_extrinsics=...): need the extrinsics of C = %d cameras, shared or for each of S = %d rigs"
                                     % (cameras, S))
        if eval_into is not None:
            from . import evaluation

            if pose_K is None:
                raise _lib.CofiError("forward_async(eval_into=...): the monitors read the submission's poses - pass pose_K")
            evaluation.check_eval_into(eval_into, B, img.device)
        if fuse_into is not None:
            from . import fusion

            if pose_K is None:
                raise _lib.CofiError("forward_async(fuse_into=...): the fusion reads the submission's poses - pass pose_K")
            rows = pc_data_dict["points"][0].shape[0]
            want = (S, rows // S, B, img.shape[-2], img.shape[-1], img.shape[-3])
            if not isinstance(fuse_into, fusion.FusionBuffers) or rows % S or not fuse_into.fits(*want, img.device):
                raise _lib.CofiError("forward_async(fuse_into=...): need a fusion.FusionBuffers made for (S, N, F, H, W, Ci) = %s on %s"
                                     % (want, img.device))
        inputs = ForwardInputs.prepare(pc_data_dict, img, inputs_stable=inputs_stable)
        # submissions in flight fill the GPU by themselves: the per-submission graph is a linear chain (intra-frame
        # fork/join only adds join latency then — measured 254 vs 331 frames/s at two frames in flight)
        with ops.arithmetic(self.arithmetic):
            outs = self._graph_forward(self._pack(img.device), inputs, mode, slot=slot, branch_mask=self.async_branch_mask,
                                       inputs_stable=inputs_stable, cameras=cameras, subpixel=subpixel)
        own = self._slots.get((slot, str(img.device)))
        if own is None:
            own = self._slots[(slot, str(img.device))] = _Slot()
        host = own.count_host.get(B)
        if host is None:
            host = own.count_host[B] = torch.empty((B, 2), dtype=torch.int32, pin_memory=True)
        host.copy_(outs[0]["count_all"], non_blocking=True)
        pose = rig_pose = None
        if pose_K is not None:
            pose, K_dev, rig_pose = own.pose.enqueue(outs, pose_K, pose_iterations, pose_seed, cameras, rig_extrinsics, pose_cov)
        if eval_into is not None:   # the evaluation monitors of the submission: one launch behind the pose tail
            evaluation.eval_monitors({"out": outs, "pose": pose}, K_dev, eval_into[1], eval_into[0], eval_into[2])
        if fuse_into is not None:   # the registered cloud of the submission: four launches behind the pose tail
            im = inputs.img.reshape((-1,) + tuple(img.shape[-3:]))
            fusion.fuse_into(inputs.points[0], im, pose, K_dev, fuse_into, result=pose["result"], cameras=cameras,
                             k_scale=float(im.shape[3]) / float(4 * (im.shape[3] // 8)))
        handle = {"out": outs, "count_host": host, "done": torch.cuda.Event()}
        handle["done"].record()
        handle.update((k, v) for k, v in (("fusion", fuse_into), ("pose", pose), ("rig_pose", rig_pose)) if v is not None)
        return handle

    @staticmethod
    def _check_rig(pc_data_dict, B, cameras) -> int:
        """the shape rules of a rig submission (cameras > 1) of B images, checked before anything is enqueued -> S, its clouds"""
        if not isinstance(cameras, int) or cameras < 1:
            raise _lib.CofiError("forward_async: cameras must be an integer >= 1, got %r" % (cameras,))
        if cameras == 1:
            return B
        if B % cameras:
            raise _lib.CofiError("forward_async: B = %d images are no whole number of rigs of C = %d cameras" % (B, cameras))
        S = B // cameras
        named = [("%s[%d]" % (k, i), t) for k in ("points", "neighbors", "subsampling", "upsampling") for i, t in enumerate(pc_data_dict[k])]
        named += [("order[%d]" % i, t) for i, t in enumerate(pc_data_dict.get("order") or [])] + [("feats", pc_data_dict["feats"])]
        for name, t in named:
            if t.shape[0] % S:
                raise _lib.CofiError("forward_async: B = %d images with C = %d cameras are S = %d clouds, which does not divide the %d rows of %s"
                                     % (B, cameras, S, t.shape[0], name))
        return S

    @torch.no_grad()
    def forward_val_async(self, slot: int, pc_data_dict, img, fine_center_kpt_coors, fine_pc_inline_index, inputs_stable: bool = False,
                          cameras: int = 1):
        """The validation pass's forward (train.py:68-70: model.eval(), mode='val') for B frames as ONE stack-mode submission on the
        current stream, through the hipGraph of slot `slot` (per slot and input signature; the labels are part of the staged inputs).
        `img` (B,3,H,W) with a stack-mode `pc_data_dict` (see stack_frames); fine_center_kpt_coors (B, 2, K) and fine_pc_inline_index
        (B, K): int64 or int32 DEVICE tensors, frame-local, read by the gather kernel without a host copy.  Returns at once with a handle:
        handle["out"][f] holds frame f's views (img_desc, pc_desc, img_score, pc_score, patches (K, C2, 4, 4), fine_pc (K, C2)),
        handle["out"][0] also the submission-wide tensors validation.val_monitors reads in place (patches_all (B, K, C2, 16), fine_pc_all
        (B, K, C2), ...); `finish_val(handle)` synchronises on this submission and returns the reference's tuples.  Slots, their reuse and
        inputs_stable are those of forward_async.  Inference only: a module in train() mode is refused (batch statistics belong to
        forward(mode='val') there), and mode='train' keeps refusing B > 1.  cameras: accepted to be refused - a rig (cameras > 1) is served
        by forward_async(mode='test') only."""
        if cameras != 1:
            raise ValueError("forward_val_async: a rig (cameras = %r) is served by forward_async(mode='test') only; validation labels are per "
                             "(cloud, image) pair - repeat the cloud per image" % (cameras,))
        if self.training:
            raise ValueError("forward_val_async is the eval()-mode validation pass (train.py:37): call model.eval() first")
        _lib.load()
        labels = []
        for name, t, shape in (("fine_center_kpt_coors", fine_center_kpt_coors, (img.shape[0], 2)), ("fine_pc_inline_index", fine_pc_inline_index, (img.shape[0],))):
            if not torch.is_tensor(t) or not t.is_cuda or t.dim() != len(shape) + 1 or tuple(t.shape[:-1]) != shape:
                raise _lib.CofiError("forward_val_async: %s must be a device tensor of shape %s + (K,)" % (name, shape))
            if t.dtype not in (torch.int64, torch.int32):
                raise _lib.CofiError("forward_val_async: %s must be int64 or int32, got %s" % (name, t.dtype))
            if inputs_stable and not t.is_contiguous():
                raise _lib.CofiError("inputs_stable=True reads the labels in place: contiguous int64 / int32 tensors only (%s)" % name)
            labels.append(t.contiguous())
        if labels[0].dtype != labels[1].dtype:
            if inputs_stable:
                raise _lib.CofiError("inputs_stable=True reads the labels in place: one integer dtype for both")
            labels = [t.to(torch.int64) for t in labels]
        inputs = ForwardInputs.prepare(pc_data_dict, img, labels, inputs_stable)   # as forward_async: stable inputs are read in place
        with ops.arithmetic(self.arithmetic):
            outs = self._graph_forward(self._pack(img.device), inputs, "val", slot=slot, branch_mask=self.async_branch_mask,
                                       inputs_stable=inputs_stable)
        done = torch.cuda.Event()
        done.record()
        return {"out": outs, "done": done, "mode": "val"}

    def finish_val(self, handle):
        """-> the reference's 8-tuple (mode='val': the last two entries are None) for every frame of a forward_val_async submission.
        The tensors are views of the slot's static outputs, valid until the slot is reused."""
        handle["done"].synchronize()
        return [(o["img_desc"], o["pc_desc"], o["img_score"], o["pc_score"], o["patches"], o["fine_pc"], None, None) for o in handle["out"]]

    def _slice_result(self, o, n: int, thr_i: int):
        if thr_i < 0:
            raise RuntimeError("fewer than 4 coarse matches at every threshold (network.py:148 would loop forever)")
        self.last_match = {"n": n, "sel": o["sel"][:n], "coarse_xy": o["coarse_xy"][:, :n], "count_dev": o["count"],
                           "fine_xy": o["fine_xy"][:, :n], "fine_best": o["fine_best"][:n], "threshold": float(score_thresholds()[thr_i])}
        return (o["img_desc"], o["pc_desc"], o["img_score"], o["pc_score"], o["patches"][:n], o["fine_pc"][:n], o["coarse_xy"][:, :n] * 4,
                o["coarse_pts"][:n])

    def finish(self, handle, per_frame_errors: bool = False):
        """-> the reference's 8-tuple for a single-frame submission, or a list of B 8-tuples for a stack-mode one
        (`handle["fine_xy"]` then holds the per-frame fine matches).  A frame with fewer than 4 coarse matches at every threshold raises
        (the reference would loop forever, network.py:148); with per_frame_errors=True the exception is RETURNED in that frame's place
        instead, so the other frames of a stack-mode submission keep their results (serving.FrameBatcher)."""
        handle["done"].synchronize()
        res, fine, per_frame = [], [], []
        for f, o in enumerate(handle["out"]):
            try:
                res.append(self._slice_result(o, int(handle["count_host"][f, 0]), int(handle["count_host"][f, 1])))
            except RuntimeError as e:
                if not per_frame_errors:
                    raise
                res.append(e)
                fine.append(None)
                per_frame.append(None)
                continue
            fine.append(self.last_match["fine_xy"])
            per_frame.append(self.last_match)
        handle["fine_xy"] = fine
        self.last_match_frames = per_frame   # stack mode: one last_match record per frame
        return res[0] if len(res) == 1 else res

    def forward(self, pc_data_dict, img, fine_center_kpt_coors, fine_xy, fine_pc_inline_index, mode, taps=None, cameras: int = 1):
        """model/network.py:74-164.  ``fine_xy`` is unused (as in the reference).

        TRAINING (train.py:224-226 followed by loss.backward(), train.py:285): mode='train' with autograd enabled - or mode 'train' /
        'val' on a module in train() mode - runs `train_forward.forward_train`: the same network as a torch.autograd graph over this
        module's parameters whose operators (every weight contraction, the KPConv aggregation, attention, the neighbour gathers) are
        HIP kernels in both directions; BatchNorm of the up-sampler then uses batch statistics and updates its running buffers, as the
        reference's module does under train(); opt.norm == 'bn': the point encoder's BatchNorm1d layers likewise (train_forward._Norm).
        INFERENCE: everything else - evaluation/eval_all.py, train.py's validation pass (test_acc, train.py:27-70: model.eval() and
        mode='val', with autograd still enabled there - nothing requires grad, so it lands here) - runs the fused, folded kernel sequence (optionally a hipGraph) and returns tensors without a
        graph.  mode='test' is never differentiable (its match selection is a host-visible count, network.py:145-151): inputs that
        require grad are refused there instead of silently losing their gradient.  cameras: accepted to be refused - a rig (one cloud under
        several images) is a forward_async submission."""
        if cameras != 1:
            raise ValueError("forward() evaluates one (cloud, image) pair per call: a rig (cameras = %r) is served by forward_async(..., cameras=C)" % (cameras,))
        if mode in ("train", "val") and (self.training or (mode == "train" and torch.is_grad_enabled())
                                         or (torch.is_grad_enabled() and (img.requires_grad or pc_data_dict["feats"].requires_grad))):
            from . import train_forward

            self._trained = True
            # gradients amplify the arithmetic's rounding (measured on the tiny frame: the 3-term bf16 split's 2^-16 per product becomes
            # up to 1e-2 in a parameter gradient; the fp32-grade arithmetics stay at the reference's own fp32 level): training computes
            # in "bf16x6" unless the module was built with an explicit arithmetic
            with ops.arithmetic(self.arithmetic if self.arithmetic is not None else "bf16x6"):
                return train_forward.forward_train(self, pc_data_dict, img, fine_center_kpt_coors, fine_pc_inline_index)
        if torch.is_grad_enabled() and (img.requires_grad or pc_data_dict["feats"].requires_grad):
            raise NotImplementedError("mode='test' is not differentiable (host-side match selection, network.py:145-151): call it under "
                                      "torch.no_grad(); gradients flow through mode='train'")
        if self.training and self.pc_norm_kind == "bn":
            raise NotImplementedError("mode='test' on a module in train() mode with opt.norm == 'bn': the inference sequence folds BatchNorm on its "
                                      "running statistics - call module.eval() (evaluation/eval_all.py does), or mode 'train' / 'val' for batch statistics")
        with torch.no_grad(), ops.arithmetic(self.arithmetic):
            return self._forward(pc_data_dict, img, fine_center_kpt_coors, fine_pc_inline_index, mode, taps)

    def _forward(self, pc_data_dict, img, fine_center_kpt_coors, fine_pc_inline_index, mode, taps=None):
        if mode not in ("train", "val", "test"):
            raise ValueError("mode must be 'train', 'val' or 'test'")
        if not img.is_cuda:
            raise _lib.CofiError("CoFiI2P.forward needs CUDA (HIP) tensors: there is no CPU path")
        _lib.load()
        P = self._pack(img.device)
        # optional keys of the pyramid: "order", the spatially sorted processing order per stage (preprocess.morton_order), and
        # "sorted_tables", the promise of sorted neighbour rows (preprocess.build_pyramid)
        i = ForwardInputs.prepare(pc_data_dict, img, (fine_center_kpt_coors, fine_pc_inline_index))
        auto = self._auto_graphs and not self._use_graphs and taps is None
        if (self._use_graphs or auto) and taps is None:
            o = self._graph_forward(P, i, mode)[0]
        else:
            o = self._run_device(P, i.points, i.neighbors, i.subsampling, i.upsampling, i.feats, i.img, mode, i.kpt, i.inl, taps=taps,
                                 order=i.order or None, sorted_tables=i.sorted_tables)[0]
        own = (lambda t: t.clone() if torch.is_tensor(t) else t) if auto else (lambda t: t)   # unasked graphs: results the caller owns
        if mode in ("train", "val"):
            return tuple(own(t) for t in (o["img_desc"], o["pc_desc"], o["img_score"], o["pc_score"], o["patches"], o["fine_pc"])) + (None, None)
        n, thr_i = (int(v) for v in o["count"].cpu())  # the only device->host synchronisation of forward
        res = self._slice_result(o, n, thr_i)
        if auto:
            self.last_match = {k_: own(v_) for k_, v_ in self.last_match.items()}
            res = tuple(own(t) for t in res)
        return res


def fine_matching(fine_img_feature_patch, fine_pc_inline_feature, fine_center_xy):
    """The fine point/pixel matching the reference performs in its callers
    (evaluation/eval_all.py:99-105, train.py:272-278): returns (fine_xy (2,n), predict_index (n,))."""
    n = fine_img_feature_patch.shape[0]
    patches = fine_img_feature_patch.reshape(n, fine_img_feature_patch.shape[1], 16).contiguous()
    cnt = torch.tensor([n, 0], dtype=torch.int32, device=patches.device)
    xy = fine_center_xy.to(torch.float32).contiguous()
    fxy, best = ops.fine_match(patches, fine_pc_inline_feature.contiguous(), xy, cnt, 1.0)
    return fxy, best.to(torch.int64)


# ---------------------------------------------------------------- free functions of model/network.py
def square_distance(src, tgt, normalize: bool = False):
    """network.py:228-247 on (B,N,3)/(B,M,3) CUDA tensors (GEMM kernel + canonical expansion)."""
    if normalize:
        raise NotImplementedError("normalize=True is never used by the reference's callers")
    out = []
    for b in range(src.shape[0]):
        s, t = src[b].contiguous(), tgt[b].contiguous()
        s4 = torch.zeros((s.shape[0], 4), device=s.device)
        t4 = torch.zeros((t.shape[0], 4), device=t.device)
        s4[:, :3], t4[:, :3] = s, t
        d = ops.gemm(s4, t4) * -2.0
        d += (s * s).sum(-1)[:, None]
        d += (t * t).sum(-1)[None, :]
        out.append(d.clamp_min(1e-12))
    return torch.stack(out)


def point2node(nodes, points):
    """network.py:250-264 -> (N,) int64 index of the nearest node (lowest index on ties)."""
    return ops.nearest_node(nodes.contiguous(), points.contiguous()).to(torch.int64)


def fine_process(coarse_pc_score, coarse_pc_feature, coarse_img_feature, thrs: float = 0.9):
    """network.py:167-187: returns (coarse_xy (2,n), pc_inline_index (n,) int64)."""
    C, H8, W8 = coarse_img_feature.shape[1:]
    pc_tok = ops.transpose(coarse_pc_feature.contiguous())
    img_tok = ops.transpose(coarse_img_feature.reshape(C, H8 * W8).contiguous())
    pix = ops.row_argmin_1m(ops.gemm(pc_tok, img_tok))
    sel, xy, cnt = ops.select_matches(coarse_pc_score.reshape(-1).contiguous(), pix, W8, H8, np.asarray([thrs], dtype=np.float32), 0)
    n = int(cnt[0])
    return xy[:, :n], sel[:n].to(torch.int64)


def extract_patch(feature_map, center_points, size: int = 4):
    """network.py:206-226: (B,C,H,W), (2,n) -> (n,B,C,4,4)."""
    if size != 4:
        raise NotImplementedError("the reference asserts 4x4 patches (network.py:222)")
    n = center_points.shape[1]
    B, C, H2, W2 = feature_map.shape
    cnt = torch.tensor([n, 0], dtype=torch.int32, device=feature_map.device)
    ctr = center_points.to(torch.float32).contiguous()
    out = []
    for b in range(B):
        nhwc = ops.transpose(feature_map[b].reshape(C, H2 * W2).contiguous())   # (H2*W2, C) pixel-major, as the forward keeps its maps
        out.append(ops.extract_patches_nhwc(nhwc, H2, W2, ctr, cnt, n, 1.0).reshape(n, C, 4, 4))
    return torch.stack(out, 1)


class CoFiI2P_wrapper(nn.Module):
    """network.py:267-274."""

    def __init__(self, opt):
        super().__init__()
        self.cofii2p = CoFiI2P(opt)

    def forward(self, inputs):
        return self.cofii2p.forward(*inputs)
