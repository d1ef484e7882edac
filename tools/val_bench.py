#!/usr/bin/env python
"""What train.py's validation pass (test_acc, train.py:27-106) costs, the parent's way against validation.validate().  GPU tool:

    python tools/val_bench.py [--out profiles/val_bench.json] [--points 20480] [--kpt 64]

Six KITTI-shaped synthetic frames (bench.make_inputs / bench.train_labels: 20480 points, 160 x 512 image, num_kpt = 64 labels), both ways
on the same box, wall-clock around a synchronised region (the baseline's time IS host time: its loop blocks on device-to-host reads),
median of repeated regions after warm-up, the two ways ALTERNATING region by region:
  (a) baseline_ms   six synchronous model.forward(mode='val') calls, each followed by what train.py:72-101 does: the caller's torch
                    expressions and test_acc's host loop (torch.nonzero + .tolist(), K x 15 list-membership tests)
  (b) validate_ms   validation.validate(): one stack-mode val submission + one cofi_val_monitors launch + one device-to-host copy
plus the split of (a) into forwards and caller code, the test-mode stack time of the same six frames (forward_async) for comparison,
and GPU dispatch counts (hipGraph nodes of a capture of each way's device part).  One JSON line, also written to --out."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import bench
from cofii2p_amd.network import CoFiI2P
from cofii2p_amd.validation import validate


def caller_device_part(outs, pc, lab, opt):
    """What a user's torch code computes on the device per frame before test_acc's host loop (train.py:72-92): key-point columns of the
    two descriptor maps, projected key points, the correspondence mask, the distance matrix, its masked copy and the row-wise sort."""
    img_desc, pc_desc = outs[0], outs[1]
    W8 = img_desc.shape[3]
    kp, ci = lab["pc_kpt_idx"], lab["coarse_img_kpt_idx"]
    img_cols = img_desc.reshape(img_desc.shape[1], -1)[:, ci]                 # (C, K)
    pc_cols = pc_desc[:, kp]                                                  # (C, K)
    cam = lab["P"][:3, :3] @ pc["points"][-1][kp].T + lab["P"][:3, 3:]
    uvw = lab["K_4"] @ cam
    pc_xy = uvw[:2] / uvw[2:]
    img_xy = torch.stack([ci % W8, ci // W8]).to(pc_xy.dtype)
    mask = ((img_xy[:, :, None] - pc_xy[:, None, :]).square().sum(0).sqrt() <= opt.dist_thres).to(pc_xy.dtype)
    dist = 1 - (img_cols[:, :, None] * pc_cols[:, None, :]).sum(0)
    return dist, mask * dist, torch.sort(dist, dim=-1).values


def caller_statements(outs, pc, lab, opt, topk_list, count, topk_range=5):
    """One frame of the parent's way: the device part above, then test_acc's host loop with ITS synchronisation pattern (train.py:90-101) -
    one nonzero, one .tolist() of the true values, and for every k and every row a .tolist() of the row's first k sorted values whose
    members are looked up in the python list -> the number of true values"""
    dist, masked, ranked = caller_device_part(outs, pc, lab, opt)
    where = torch.nonzero(masked)
    true_values = masked[where[:, 0], where[:, 1]].tolist()
    for k in range(1, topk_range + 1):
        head = ranked[:, :k]
        for r in range(head.shape[0]):
            topk_list[count, k - 1] += sum(1 for v in head[r].tolist() if v in true_values)
    return len(true_values)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "val_bench.json"))
    ap.add_argument("--points", type=int, default=20480)
    ap.add_argument("--kpt", type=int, default=64)
    ap.add_argument("--regions", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("val_bench needs a GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    model = CoFiI2P(bench.Opt()).to(dev)
    model.eval()
    frames = bench.make_inputs(dev, list(range(6)), args.points)
    labs = [bench.train_labels(pyr, dev, num_kpt=args.kpt, seed=f) for f, (pyr, _img, _fr) in enumerate(frames)]
    samples = []
    for (pyr, img, _fr), lab in zip(frames, labs):
        s = {"img": img, "pc_data_dict": pyr}
        s.update({k: v for k, v in lab.items() if k != "fine_xy"})
        s["fine_xy_coors"] = lab["fine_xy"]
        samples.append(s)
    opt = bench.StepOpt
    split = {"forward": [], "caller": []}

    def baseline(record=False):
        topk_list = torch.zeros(6, 5)
        n = 1
        for count, ((pyr, img, _fr), lab) in enumerate(zip(frames, labs)):
            t0 = time.perf_counter()
            outs = model(pyr, img, lab["fine_center_kpt_coors"], lab["fine_xy"], lab["fine_pc_inline_index"], "val")
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            n = caller_statements(outs, pyr, lab, opt, topk_list, count)
            if record:
                split["forward"].append(t1 - t0), split["caller"].append(time.perf_counter() - t1)
        return torch.mean(topk_list / n, dim=0)

    def new():
        return validate(model, samples, opt, slot=0)["acc"]

    def region(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    for _ in range(3):   # warm-up: workspaces, the val graph's capture, torch's lazy initialisations
        acc_a, acc_b = baseline(), new()
    ta, tb = [], []
    for _ in range(args.regions):   # alternate: what shares the box with this process moves both
        ta.append(region(lambda: baseline(True))[0])
        tb.append(region(new)[0])
    # the test-mode stack rate of the same six frames, for comparison (forward_async + finish)
    stacked, imgs = CoFiI2P.stack_frames([f[0] for f in frames], [f[1] for f in frames])
    tt = []
    for i in range(3 + args.regions):
        t, _ = region(lambda: model.finish(model.forward_async(1, stacked, imgs), per_frame_errors=True))
        if i >= 3:
            tt.append(t)
    # GPU dispatches, counted as hipGraph nodes of a capture (bench.graph_node_census): the new way's whole device part (stacked val forward +
    # monitors), the baseline's per-frame val forward and the device part of its caller code (its host loop cannot be captured: it syncs)
    from cofii2p_amd.validation import stack_labels, val_monitors

    labels = stack_labels(labs)
    P_b = model._pack(dev)
    with torch.no_grad():
        def new_device():
            outs = model._run_device(P_b, stacked["points"], stacked["neighbors"], stacked["subsampling"], stacked["upsampling"], stacked["feats"],
                                     imgs, "val", labels["fine_center_kpt_coors"], labels["fine_pc_inline_index"])
            return val_monitors(outs, labels, opt)

        pyr0, img0, lab0 = frames[0][0], frames[0][1], labs[0]

        def one_forward():
            return model._run_device(P_b, pyr0["points"], pyr0["neighbors"], pyr0["subsampling"], pyr0["upsampling"], pyr0["feats"], img0, "val",
                                     lab0["fine_center_kpt_coors"], lab0["fine_pc_inline_index"])

        o0 = one_forward()[0]
        outs0 = (o0["img_desc"], o0["pc_desc"])
        census = {}
        for name, fn in (("validate_device_part", new_device), ("baseline_one_forward", one_forward),
                         ("baseline_caller_device_part_one_frame", lambda: caller_device_part(outs0, pyr0, lab0, opt))):
            try:
                census[name] = bench.graph_node_census(fn)
            except Exception as e:   # a count that could not be taken is reported as such; the timings above stand
                census[name] = "not counted: %s" % type(e).__name__
                torch.cuda.synchronize()
    rec = {"tool": "tools/val_bench.py", "device": torch.cuda.get_device_name(0), "frames": 6, "points": args.points, "num_kpt": args.kpt,
           "arithmetic": model.arithmetic or "library default", "timing": "wall clock around synchronised regions, median of %d alternating regions after 3 warm-up rounds" % args.regions,
           "baseline_ms": round(statistics.median(ta), 3), "baseline_ms_regions": [round(v, 3) for v in ta],
           "baseline_forward_ms": round(1e3 * 6 * statistics.median(split["forward"]), 3), "baseline_caller_ms": round(1e3 * 6 * statistics.median(split["caller"]), 3),
           "validate_ms": round(statistics.median(tb), 3), "validate_ms_regions": [round(v, 3) for v in tb],
           "test_mode_stack_ms": round(statistics.median(tt), 3),
           "speedup": round(statistics.median(ta) / statistics.median(tb), 2),
           "same_acc": bool(torch.equal(acc_a, acc_b)), "acc_baseline": [float(v) for v in acc_a], "acc_validate": [float(v) for v in acc_b],
           "graph_nodes": census,
           "host_syncs": {"validate": 1, "baseline_per_frame": 1 + 1 + 1 + 5 * args.kpt,
                          "baseline_per_frame_what": "forward's sync + nonzero + true-value .tolist() + 5 x num_kpt candidate .tolist() reads"}}
    line = json.dumps(rec)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
