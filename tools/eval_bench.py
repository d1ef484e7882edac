#!/usr/bin/env python
"""What scoring a validation set costs on top of the stack-mode pipeline, the parent's way against evaluation.evaluate().  GPU tool:

    python tools/eval_bench.py [--out profiles/eval_bench.json] [--frames 64] [--batch 16] [--points 20480]

The bench's synthetic frames (bench.make_inputs: 20480 points, 160 x 512 image) with a made-up camera and rigid ground-truth pose per
frame, three loops in one process, wall clock around a synchronised region, median of repeated regions after warm-up, the three loops
ALTERNATING region by region; frames/s of
  (a) pipeline   FrameBatcher(pose=True) alone: frames in, poses out, nothing scored
  (b) host       the parent's way: (a) plus, per frame, what a user's eval_all.py-shaped loop does with the tools the package had -
                 pose.pose_matrix (R, t read back), pose.get_P_diff and metrics.inlier_ratio_rmse (fine_xy, points read back) on the host
  (c) evaluate   evaluation.evaluate(): the monitors of a stack in one launch behind its poses, one device-to-host copy at the end
and the distance of (c) from (a) next to the spread of (a)'s own regions.  One JSON line, also written to --out."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import bench
from cofii2p_amd import metrics, pose
from cofii2p_amd.evaluation import evaluate
from cofii2p_amd.network import CoFiI2P
from cofii2p_amd.serving import FrameBatcher


def made_up(i):
    """a camera and a rigid ground-truth pose for frame i (float32, as a loader hands them over)"""
    K = np.array([[300.0 + (i % 7), 0, 256.0], [0, 296.0 + (i % 5), 80.0], [0, 0, 1.0]], np.float32)
    a, b, c = np.radians([3.0 * (i % 9), 5.0 - (i % 4), 2.0 + (i % 3)])
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    Rz = np.array([[np.cos(b), -np.sin(b), 0], [np.sin(b), np.cos(b), 0], [0, 0, 1]])
    Ry = np.array([[np.cos(c), 0, np.sin(c)], [0, 1, 0], [-np.sin(c), 0, np.cos(c)]])
    P = np.eye(4)
    P[:3, :3], P[:3, 3] = Ry @ Rz @ Rx, [0.5 * (i % 4), -0.2, 1.0 + 0.1 * (i % 6)]
    return K, P.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_bench.json"))
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--distinct", type=int, default=16, help="distinct synthetic frames (cycled)")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--streams", type=int, default=4)
    ap.add_argument("--points", type=int, default=20480)
    ap.add_argument("--iterations", type=int, default=10000)
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_bench needs a GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    model = CoFiI2P(bench.Opt()).to(dev)
    model.eval()
    model.enable_graphs(True)
    distinct = bench.make_inputs(dev, list(range(args.distinct)), args.points)
    N = args.frames
    KP = [made_up(i) for i in range(N)]
    samples = [{"pc_data_dict": distinct[i % args.distinct][0], "img": distinct[i % args.distinct][1],
                "K": torch.from_numpy(KP[i][0]).to(dev), "P": torch.from_numpy(KP[i][1]).to(dev)} for i in range(N)]
    K64 = [k.astype(np.float64) for k, _ in KP]
    P64 = [p.astype(np.float64) for _, p in KP]
    fb = FrameBatcher(model, batch=args.batch, streams=args.streams, slot_base=200, pose=True, pose_iterations=args.iterations)

    def pipeline(score):
        """(a) / (b): tickets are read out one stack behind the submissions, as a pipelined caller does"""
        t_err, r_err, irs = [], [], []
        tickets = []

        def read(lo, hi):
            for i in range(lo, hi):
                try:
                    out = fb.result(tickets[i])
                except RuntimeError:
                    continue
                res, R, t, _inl = fb.pose_result(tickets[i])
                if not score:
                    continue
                if int(res[0]):
                    d = pose.get_P_diff(pose.pose_matrix(R, t), P64[i])
                    t_err.append(d[0]), r_err.append(d[1])
                irs.append(metrics.inlier_ratio_rmse(fb.fine_xy(tickets[i]).cpu().numpy().astype(np.float64), out[7].cpu().numpy().astype(np.float64),
                                                     P64[i], K64[i]))
        done = 0
        for i, s in enumerate(samples):
            tickets.append(fb.submit(s["pc_data_dict"], s["img"], K=s["K"]))
            if (i + 1) % args.batch == 0 and i + 1 >= 2 * args.batch:
                read(done, done + args.batch)
                done += args.batch
        fb.drain()
        read(done, N)
        return t_err, r_err, irs

    def new():
        return evaluate(model, samples, None, batch=args.batch, streams=args.streams, pose_iterations=args.iterations, slot_base=300)

    def region(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return N / (time.perf_counter() - t0), r

    for _ in range(args.warmup):   # graph captures of every stack of every loop, workspaces, torch's lazy initialisations
        pipeline(False), pipeline(True), new()
    fa, fbs, fc = [], [], []
    for _ in range(args.regions):   # alternate: what shares the box with this process moves all three
        fa.append(region(lambda: pipeline(False))[0])
        rate, host = region(lambda: pipeline(True))
        fbs.append(rate)
        rate, dev_res = region(new)
        fc.append(rate)
    a, b, c = statistics.median(fa), statistics.median(fbs), statistics.median(fc)
    same = bool(len(host[0]) == len(dev_res["t_error"]) and np.allclose(host[0], dev_res["t_error"], rtol=1e-7, atol=1e-9)
                and np.allclose(host[1], dev_res["r_error"], rtol=1e-7, atol=1e-7))
    rec = {"tool": "tools/eval_bench.py", "device": torch.cuda.get_device_name(0), "frames": N, "distinct_frames": args.distinct, "batch": args.batch,
           "streams": args.streams, "points": args.points, "pose_iterations": args.iterations, "arithmetic": model.arithmetic or "library default",
           "timing": "wall clock around synchronised regions, median of %d alternating regions after %d warm-up rounds" % (args.regions, args.warmup),
           "pipeline_fps": round(a, 1), "pipeline_fps_regions": [round(v, 1) for v in fa],
           "host_scoring_fps": round(b, 1), "host_scoring_fps_regions": [round(v, 1) for v in fbs],
           "evaluate_fps": round(c, 1), "evaluate_fps_regions": [round(v, 1) for v in fc],
           "evaluate_over_host_scoring": round(c / b, 3),
           "evaluate_vs_pipeline_percent": round(100.0 * (c - a) / a, 2),
           "pipeline_spread_percent": round(100.0 * (max(fa) - min(fa)) / a, 2),
           "same_errors_as_host_scoring": same,
           "host_syncs": {"evaluate": "one device-to-host copy of the table (plus the count copy every submission already makes)",
                          "host_scoring_per_frame": "R, t, fine_xy and coarse points read back"}}
    line = json.dumps(rec)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
