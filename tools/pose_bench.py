#!/usr/bin/env python
"""What the pose of a stack-mode submission costs, per-frame calls against the batched pass.  GPU tool:

    python tools/pose_bench.py [--out profiles/pose_batch.json] [--no-pipeline]

B = 16 frames of synthetic correspondences (tests/test_pose_cpu.py::synth restated: ~400 valid rows in buffers of cap = 1280, 40 %
outliers, 1 px noise), 10 000 hypotheses, HIP-event times after warm-up, median of repeated regions:
  (a) per_frame_16_ms   16 calls of pose.solve_pnp_ransac (the per-frame entry, untouched) on one stream
  (b) batched_16_ms     one pose.solve_pnp_ransac_batch call reading (B,cap,3) / (B,2,cap) / count / K in place
  (c) batched_ms        the batched call for B = 1, 4, 16, 32
and frames/s of a serving.FrameBatcher loop (batch 16, the bench's synthetic KITTI-shaped frames) with the pose off, on (batched tail
behind every forward) and done by per-frame calls on every ticket's result.  One JSON line, also written to --out."""
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

from cofii2p_amd import pose

K_CAM = np.array([[700.0, 0, 256.0], [0, 700.0, 80.0], [0, 0, 1.0]])
CAP, ITERS = 1280, 10000


def synth(rng, n, noise=1.0, outliers=0.4):
    w = rng.normal(size=3) * 0.4
    th = np.linalg.norm(w)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
    t = rng.normal(size=3) * 2 + np.array([0, 0, 12.0])
    X = rng.uniform(-20, 20, (n, 3))
    X[:, 2] = rng.uniform(-5, 5, n)
    Y = X @ R.T + t
    uv = np.stack([K_CAM[0, 0] * Y[:, 0] / Y[:, 2] + K_CAM[0, 2], K_CAM[1, 1] * Y[:, 1] / Y[:, 2] + K_CAM[1, 2]], 1) + rng.normal(size=(n, 2)) * noise
    out = rng.random(n) < outliers
    uv[out] = rng.uniform(0, 512, (int(out.sum()), 2))
    return X.astype(np.float32), uv.astype(np.float32)


def make_batch(B, dev, seed=0):
    rng = np.random.default_rng(seed)
    X, uv, counts = np.zeros((B, CAP, 3), np.float32), np.zeros((B, CAP, 2), np.float32), []
    for f in range(B):
        n = int(rng.integers(360, 441))
        X[f, :n], uv[f, :n] = synth(rng, n)
        counts.append(n)
    Xd, uvd = torch.from_numpy(X).to(dev), torch.from_numpy(uv).to(dev)
    return (Xd, uvd.transpose(1, 2).contiguous(), torch.from_numpy(np.stack([K_CAM] * B).astype(np.float32)).to(dev),
            torch.tensor(counts, dtype=torch.int32, device=dev), [(Xd[f, :n].contiguous(), uvd[f, :n].contiguous()) for f, n in enumerate(counts)])


def event_ms(fn, calls=20, regions=9, warmup=5):
    """median over `regions` event-timed regions of `calls` back-to-back calls -> (ms per call, [min, max] of the regions)"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    per = []
    for _ in range(regions):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        e1.synchronize()
        per.append(e0.elapsed_time(e1) / calls)
    return statistics.median(per), [min(per), max(per)]


def batcher_rates(dev, stacks=24, warm=10):
    """frames/s of a FrameBatcher loop over the bench's synthetic frames: results of a stack are read while the next ones are in flight"""
    import bench
    from cofii2p_amd.network import CoFiI2P
    from cofii2p_amd.serving import FrameBatcher

    B = 16
    model = CoFiI2P(bench.Opt()).to(dev)
    model.enable_graphs(True)
    frames = bench.make_inputs(dev, list(range(B)), 20480)
    Kc = np.array([[300.0, 0, 256.0], [0, 300.0, 80.0], [0, 0, 1.0]])
    Kd = torch.from_numpy(Kc.astype(np.float32)).to(dev)
    fb = FrameBatcher(model, batch=B, pose=True, pose_iterations=ITERS)
    keep = []

    def consume(tickets, mode):
        for tk in tickets:
            try:
                out = fb.result(tk)
            except RuntimeError:
                continue          # a frame without matches
            if mode == "on":
                keep.append(fb.pose_result(tk))
            elif mode == "per_frame":
                keep.append(pose.solve_pnp_ransac(out[7].contiguous(), fb.fine_xy(tk).t().contiguous(), Kc, iterations=ITERS, seed=tk[2]))
            del keep[:-4]

    def loop(n_stacks, mode):
        fb.pose = mode == "on"
        pending = []
        for s in range(n_stacks):
            pending.append([fb.submit(fr[0], fr[1], K=Kd) for fr in frames])
            if len(pending) > fb.ring - 2:
                consume(pending.pop(0), mode)
        while pending:
            consume(pending.pop(0), mode)
        torch.cuda.synchronize()

    rates = {}
    for mode in ("off", "on", "per_frame"):
        loop(warm, mode)
        per = []
        for _ in range(3):
            t0 = time.perf_counter()
            loop(stacks, mode)
            per.append(stacks * B / (time.perf_counter() - t0))
        rates[mode] = {"frames_per_s": round(statistics.median(per), 1), "regions": [round(p, 1) for p in per]}
    return rates


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_batch.json"))
    ap.add_argument("--no-pipeline", action="store_true", help="skip the FrameBatcher rates")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pose_bench needs a GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    X, fxy, Ks, cnt, per_frame = make_batch(16, dev)
    rec = {"tool": "tools/pose_bench.py", "device": torch.cuda.get_device_name(0), "frames": 16, "cap": CAP, "iterations": ITERS,
           "valid_rows": [int(c) for c in cnt.cpu()], "timing": "HIP events, median of 9 regions of 20 calls after 5 warm-up calls"}

    def a():
        for f, (Xf, uvf) in enumerate(per_frame):
            pose.solve_pnp_ransac(Xf, uvf, K_CAM, iterations=ITERS, seed=f)

    def b():
        pose.solve_pnp_ransac_batch(X, fxy, Ks, count=cnt, iterations=ITERS, coord_major=True)

    # alternate the two forms: what shares the box with this process moves both
    ta1, ra1 = event_ms(a)
    tb1, rb1 = event_ms(b)
    ta2, ra2 = event_ms(a)
    tb2, rb2 = event_ms(b)
    rec["per_frame_16_ms"] = round(statistics.median([ta1, ta2]), 4)
    rec["per_frame_16_ms_regions"] = [round(v, 4) for v in ra1 + ra2]
    rec["batched_16_ms"] = round(statistics.median([tb1, tb2]), 4)
    rec["batched_16_ms_regions"] = [round(v, 4) for v in rb1 + rb2]
    rec["batched_over_per_frame"] = round(rec["batched_16_ms"] / rec["per_frame_16_ms"], 4)
    res_b = pose.solve_pnp_ransac_batch(X, fxy, Ks, count=cnt, iterations=ITERS, coord_major=True)
    res_a = [pose.solve_pnp_ransac(Xf, uvf, K_CAM, iterations=ITERS, seed=f) for f, (Xf, uvf) in enumerate(per_frame)]
    rec["same_results"] = all(torch.equal(res_b[0][f], r[0]) and torch.equal(res_b[1][f], r[1]) and torch.equal(res_b[2][f], r[2])
                              for f, r in enumerate(res_a))
    rec["batched_ms"] = {}
    for B in (1, 4, 16, 32):
        Xb, fb_, Kb, cb, _ = make_batch(B, dev, seed=B)
        rec["batched_ms"][str(B)] = round(event_ms(lambda: pose.solve_pnp_ransac_batch(Xb, fb_, Kb, count=cb, iterations=ITERS, coord_major=True))[0], 4)
    if not args.no_pipeline:
        rec["frame_batcher"] = batcher_rates(dev)
    line = json.dumps(rec)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
