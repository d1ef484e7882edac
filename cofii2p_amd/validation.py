"""The validation pass of train.py on the device.

What train.py does every `opt.val_freq` steps to tell whether training is healthy, with the host loops and per-frame launches removed:

* `test_acc` (train.py:27-106, :307-322): top-1..5 coarse-descriptor recall on the first 6 validation frames   -> `validate`
* `fine_recall` (train.py:271-281) and the `pc_score` scalars (train.py:256-259) of a training step            -> `train_monitors`

Both end in one kernel, `cofi_val_monitors` (csrc/validation.hip), which covers every frame of a submission in one launch and reads
the forward's outputs in place.  `validate` feeds it from ONE stack-mode mode='val' submission (`CoFiI2P.forward_val_async`) instead of
six synchronous single-frame forwards, and copies the results to the host once.

    acc = validate(model, testloader, opt)["acc"]          # train.py:308 - the same five numbers, as a CPU tensor

THE DIVISOR QUIRK of train.py:103.  `acc = torch.mean(topk_list / len(true_value_list), dim=0)` divides the count rows of ALL frames by
the number of true pairs of the LAST frame processed (the loop variable survives the loop), and averages over a fixed 6 rows - rows of
frames that were never processed stay zero, so 3 validation frames give half the value.  `reference_acc` reproduces exactly that,
because it is the number a user compares against the reference's logs; `frame_recall` is the plain per-frame recall
counts[f] / n_true[f], which is what the quantity means.  `validate` returns both.
"""
import itertools
from typing import Dict, Iterable, List, Optional

import torch

from . import _lib, ops
from .train_step import _PYRAMID_LISTS, batch_from_sample

__all__ = ["val_monitors", "reference_acc", "frame_recall", "validate", "train_monitors", "stack_labels"]

_INDEX_LABELS = ("pc_kpt_idx", "pc_outline_idx", "coarse_img_kpt_idx")
_PIXEL_LABELS = ("fine_xy", "fine_center_kpt_coors")


def stack_labels(batches: List[Dict[str, torch.Tensor]], device=None) -> Dict[str, torch.Tensor]:
    """B per-frame label sets (the `batch` of train_step.batch_from_sample) -> one set with a leading frame axis: index lists (B, K),
    pixel coordinates (B, 2, K), K_4 (B, 3, 3), P (B, 4, 4), on `device`."""
    dev = torch.device(device) if device is not None else batches[0]["pc_kpt_idx"].device
    keys = _INDEX_LABELS + _PIXEL_LABELS + ("fine_pc_inline_index", "K_4", "P")
    return {k: torch.stack([b[k].to(dev) for b in batches]) for k in keys if all(k in b for b in batches)}


def _frame_axis(labels: Dict[str, torch.Tensor], B: int, dev) -> Dict[str, torch.Tensor]:
    """labels as the kernel reads them: a leading frame axis, one integer dtype, float32 K_4 / P; conversions run on the device"""
    out = {}
    ints = [labels[k] for k in _INDEX_LABELS + _PIXEL_LABELS]
    dt = torch.int32 if all(t.dtype == torch.int32 for t in ints) else torch.int64
    for k in _INDEX_LABELS + _PIXEL_LABELS:
        t = labels[k]
        if not t.is_cuda:
            raise _lib.CofiError("val_monitors: label %s must be on the GPU - there is no CPU path" % k)
        if t.is_floating_point():
            raise _lib.CofiError("val_monitors: label %s must be an integer tensor" % k)
        want = 1 if k in _INDEX_LABELS else 2
        t = t[None] if t.dim() == want else t
        out[k] = t.to(dt).contiguous()
    for k, shape in (("K_4", (3, 3)), ("P", (4, 4))):
        t = labels[k].to(device=dev, dtype=torch.float32)
        t = t[None] if t.dim() == 2 else t
        if tuple(t.shape) == (1,) + shape and B > 1:
            t = t.expand(B, *shape)
        out[k] = t.contiguous()
    return out


def val_monitors(outs_or_handle, labels: Dict[str, torch.Tensor], opt, topk_range: int = 5, debug: bool = False, out: Optional[Dict] = None) -> Dict[str, torch.Tensor]:
    """The monitors of every frame of a mode='val' submission, in one launch on the current stream and with no host read.

    outs_or_handle: the handle of `CoFiI2P.forward_val_async` (or its handle["out"] list).  labels: pc_kpt_idx, pc_outline_idx,
    coarse_img_kpt_idx (B, K), fine_xy, fine_center_kpt_coors (B, 2, K) - int64 or int32 device tensors - and K_4 (B, 3, 3), P (B, 4, 4)
    (`stack_labels`); a single frame may leave the frame axis out.  opt: dist_thres.
    -> device tensors counts (B, topk_range) int32, n_true (B,) int32, fine_hits (B,) int32, score_stats (B, 6) float32 = [in-line max, min,
    mean, out-line max, min, mean] of pc_score; debug=True adds dist and mask (B, K, K)."""
    outs = outs_or_handle["out"] if isinstance(outs_or_handle, dict) and "out" in outs_or_handle else outs_or_handle
    o0 = outs[0]
    if "patches_all" not in o0:
        raise _lib.CofiError("val_monitors reads the submission-wide outputs of CoFiI2P.forward_val_async (patches_all, ...)")
    img_desc = o0["img_desc_all"]
    B, dev = img_desc.shape[0], img_desc.device
    W8 = o0["img_desc"].shape[3]
    lab = _frame_axis(labels, B, dev)
    return ops.val_monitors(img_desc, o0["pc_desc_all"], W8, o0["points4"], o0["pc_score_all"], o0["patches_all"], o0["fine_pc_all"], lab,
                            lab["K_4"], lab["P"], float(opt.dist_thres), topk=topk_range, debug=debug, out=out)


def train_monitors(outs, pc_data_dict, batch: Dict[str, torch.Tensor], opt, topk_range: int = 5, debug: bool = False) -> Dict[str, torch.Tensor]:
    """The same kernel with B = 1 on the (detached) outputs of a training step: `outs` = what the model returned for
    (pc_data_dict, img, batch) in mode 'train' / 'val' (train_step.step_losses' first result).  fine_hits[0] / num_kpt is train.py:280's
    fine_recall, score_stats[0] the six pc_score scalars of train.py:258-259; counts / n_true are test_acc's quantities for this frame."""
    with torch.no_grad():
        img_f, pc_f, _img_s, pc_s, patch, fine_pc = (t.detach() for t in outs[:6])
        C, K = img_f.shape[1], patch.shape[0]
        lab = _frame_axis(batch, 1, img_f.device)
        return ops.val_monitors(img_f.reshape(1, C, -1).contiguous(), pc_f.reshape(1, C, -1).contiguous(), img_f.shape[3],
                                pc_data_dict["points"][-1].to(torch.float32).contiguous(), pc_s.reshape(-1).contiguous(),
                                patch.reshape(1, K, -1, 16).contiguous(), fine_pc.reshape(1, K, -1).contiguous(), lab, lab["K_4"], lab["P"],
                                float(opt.dist_thres), topk=topk_range, debug=debug)


def reference_acc(counts: torch.Tensor, n_true: torch.Tensor, rows: int = 6) -> torch.Tensor:
    """train.py:31,101-103 literally: `topk_list = torch.zeros(6, topk_range)`, one count row per processed frame, then
    `torch.mean(topk_list / len(true_value_list), dim=0)` with the true list of the LAST processed frame.  counts (B, topk), n_true (B,);
    frames beyond `rows` are ignored (train.py:35-36), rows of missing frames stay zero, and a last frame without a true pair divides by
    zero the way torch does (inf / nan, no exception).  See the module docstring; `frame_recall` is the per-frame quantity."""
    b = min(int(counts.shape[0]), rows)
    topk_list = torch.zeros(rows, counts.shape[1], device=counts.device)
    if b == 0:
        raise ValueError("reference_acc: no frame (train.py:103 would raise a NameError)")
    topk_list[:b] = counts[:b].to(topk_list.dtype)
    last = n_true[b - 1]
    return torch.mean(topk_list / (int(last) if not last.is_cuda else last.to(topk_list.dtype)), dim=0)


def frame_recall(counts: torch.Tensor, n_true: torch.Tensor) -> torch.Tensor:
    """counts / n_true[:, None] as float32: of frame f's true pairs, the share found among the k smallest distances of their rows
    (by the reference's value-membership rule) - every frame divided by ITS OWN number of true pairs."""
    return counts.to(torch.float32) / n_true.to(torch.float32)[:, None]


def _size_signature(pc, img):
    return (tuple(img.shape),) + tuple(tuple(t.shape) for k in _PYRAMID_LISTS for t in pc[k]) + (tuple(pc["feats"].shape),)


def validate(model, frames: Iterable[Dict], opt, slot: int = 0, topk_range: int = 5, max_frames: int = 6, device=None) -> Dict[str, torch.Tensor]:
    """test_acc (train.py:27-106) on the device.  `frames`: an iterable of data-side samples with the fields
    train_step.batch_from_sample reads (FramePreparer / FrameLoader samples, or batches of 1 of the reference's DataLoader); the first
    `max_frames` = 6 are taken (train.py:35-36).  They go through ONE stack-mode mode='val' submission on `slot` followed by one
    `val_monitors` launch; frames of different sizes fall back to one submission per group of equally sized frames.  The module is put
    into eval() for the pass (train.py:37) and back afterwards.  One device-to-host copy at the end.

    -> CPU tensors: acc (topk_range,) = the reference's numbers (`reference_acc`), recall (B, topk_range) = `frame_recall`, counts, n_true,
    fine_hits, score_stats."""
    from .network import CoFiI2P

    dev = torch.device(device) if device is not None else next(model.parameters()).device
    triples = [batch_from_sample(s, dev) for s in itertools.islice(iter(frames), max_frames)]
    if not triples:
        raise ValueError("validate: no frame")
    groups: Dict[tuple, List[int]] = {}
    for i, (pc, img, batch) in enumerate(triples):
        groups.setdefault(_size_signature(pc, img) + (int(batch["pc_kpt_idx"].numel()),), []).append(i)
    B = len(triples)
    packed = torch.empty((B, topk_range + 2 + 6), dtype=torch.int32, device=dev)   # counts | n_true | fine_hits | score_stats (bit pattern)
    was_training = model.training
    model.eval()
    try:
        for members in groups.values():
            stacked, img = CoFiI2P.stack_frames([triples[i][0] for i in members], [triples[i][1] for i in members])
            labels = stack_labels([triples[i][2] for i in members], dev)
            handle = model.forward_val_async(slot, stacked, img, labels["fine_center_kpt_coors"], labels["fine_pc_inline_index"])
            m = val_monitors(handle, labels, opt, topk_range=topk_range)
            rows = torch.cat([m["counts"], m["n_true"][:, None], m["fine_hits"][:, None], m["score_stats"].view(torch.int32)], 1)
            if len(groups) == 1:
                packed = rows
            else:
                packed.index_copy_(0, torch.tensor(members, dtype=torch.int64).to(dev, non_blocking=True), rows)
    finally:
        model.train(was_training)
    host = packed.cpu()   # the pass's only device-to-host copy
    counts, n_true, fine_hits = host[:, :topk_range].contiguous(), host[:, topk_range].contiguous(), host[:, topk_range + 1].contiguous()
    score_stats = host[:, topk_range + 2:].contiguous().view(torch.float32)
    return {"acc": reference_acc(counts, n_true), "recall": frame_recall(counts, n_true), "counts": counts, "n_true": n_true,
            "fine_hits": fine_hits, "score_stats": score_stats}
