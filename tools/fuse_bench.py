#!/usr/bin/env python
"""What the registered cloud of a submission costs (fusion.fuse_into), alone and behind the pose tail it follows.  GPU tool:

    python tools/fuse_bench.py [--out profiles/fusion.json]

16 images of 160 x 512 against clouds of 20 480 points (the KITTI shape of bench.py) as S = 16 / 8 / 4 clouds under C = 1 / 2 / 4 cameras, splat
0 / 1 / 2.  The clouds are a ground plane, two walls and a scatter 4 - 60 m in front of the cameras, the poses small motions, so that about
a third of every cloud falls into every picture.  HIP-event times after warm-up, median of repeated regions:
  fuse_ms        fusion.fuse_into alone
  tail_ms        pose.solve_pnp_ransac_batch_into alone on ~400 synthetic matches per image (10 000 hypotheses)
  tail_fuse_ms   the pose tail with the fusion behind it, reading the poses and results the tail has just written
the three alternated in one process.  One JSON line, also written to --out."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from cofii2p_amd import fusion, pose

F, N, H, W, CAP, ITERS = 16, 20480, 160, 512, 1280, 10000
K_FULL = np.array([[600.0, 0, 255.5], [0, 600.0, 79.5], [0, 0, 1.0]])


def small_pose(rng, yaw=0.0):
    w = rng.normal(scale=0.02, size=3) + np.array([0.0, yaw, 0.0])
    th = np.linalg.norm(w)
    Kx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    R = np.eye(3) + np.sin(th) / th * Kx + (1 - np.cos(th)) / th ** 2 * Kx @ Kx
    return R, rng.normal(scale=0.2, size=3)


def make_cloud(rng):
    """camera-like frame (x right, y down, z forward): ground plane, two side walls, a scatter"""
    n = N // 4
    ground = np.stack([rng.uniform(-15, 15, n), 1.6 + rng.normal(scale=0.03, size=n), rng.uniform(3, 60, n)], 1)
    left = np.stack([-8 + rng.normal(scale=0.05, size=n), rng.uniform(-4, 1.6, n), rng.uniform(3, 60, n)], 1)
    right = np.stack([9 + rng.normal(scale=0.05, size=n), rng.uniform(-4, 1.6, n), rng.uniform(3, 60, n)], 1)
    scatter = np.stack([rng.uniform(-30, 30, N - 3 * n), rng.uniform(-6, 2, N - 3 * n), rng.uniform(-20, 60, N - 3 * n)], 1)
    return np.concatenate([ground, left, right, scatter])[rng.permutation(N)].astype(np.float32)


def scene(C, dev, seed=0):
    rng = np.random.default_rng(seed)
    S = F // C
    pts = np.stack([make_cloud(rng) for _ in range(S)])
    poses, X, uv, counts = np.zeros((F, 12), np.float32), np.zeros((F, CAP, 3), np.float32), np.zeros((F, CAP, 2), np.float32), []
    K_half = K_FULL.copy()
    K_half[:2] /= 2
    for f in range(F):
        R, t = small_pose(rng, yaw=0.25 * (f % C - (C - 1) / 2))
        poses[f] = np.concatenate([R.reshape(9), t])
        cam = pts[f // C].astype(np.float64) @ R.T + t
        px = (K_half @ cam.T).T
        px = px[:, :2] / px[:, 2:]
        ok = np.nonzero((cam[:, 2] > 1) & (px[:, 0] >= 0) & (px[:, 0] < W / 2) & (px[:, 1] >= 0) & (px[:, 1] < H / 2))[0]
        n = int(rng.integers(360, 441))
        sel = rng.choice(ok, n, replace=False)
        X[f, :n], uv[f, :n] = pts[f // C, sel], px[sel] + rng.normal(scale=0.5, size=(n, 2))
        out = rng.permutation(n)[:int(0.3 * n)]
        uv[f, out] = np.stack([rng.uniform(0, W / 2, len(out)), rng.uniform(0, H / 2, len(out))], 1)
        counts.append(n)
    y, x = np.mgrid[0:H, 0:W]
    img = np.stack([np.stack([0.5 + 0.4 * np.sin(0.02 * x + 0.05 * y + ch + f) for ch in range(3)]) for f in range(F)]).astype(np.float32)
    to = lambda a: torch.from_numpy(a).to(dev)
    return {"points": to(pts), "images": to(img), "pose_gt": to(poses), "X": to(X), "fxy": to(uv).transpose(1, 2).contiguous(),
            "K_half": to(np.stack([K_half] * F).astype(np.float32)), "count": torch.tensor(counts, dtype=torch.int32, device=dev)}


def event_ms(fn, calls=20, regions=9, warmup=5):
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


def measure(dev):
    out = {}
    for C in (1, 2, 4):
        sc = scene(C, dev, seed=C)
        S = F // C
        tail = (torch.empty(pose.pnp_batch_workspace(ITERS, F), dtype=torch.uint8, device=dev), torch.empty((F, 12), device=dev),
                torch.empty((F, 3), dtype=torch.int32, device=dev), torch.empty((F, CAP), dtype=torch.uint8, device=dev))
        buf = fusion.FusionBuffers(S, N, F, H, W, 3, dev)

        def run_tail():
            pose.solve_pnp_ransac_batch_into(sc["X"], sc["fxy"], sc["K_half"], sc["count"], *tail, iterations=ITERS, coord_major=True)

        run_tail()
        t_tail = [event_ms(run_tail) for _ in range(2)]
        for splat in (0, 1, 2):
            def fuse_gt():
                fusion.fuse_into(sc["points"], sc["images"], sc["pose_gt"], sc["K_half"], buf, cameras=C, k_scale=2.0, splat=splat)

            def tail_fuse():
                run_tail()
                fusion.fuse_into(sc["points"], sc["images"], tail[1], sc["K_half"], buf, result=tail[2], cameras=C, k_scale=2.0, splat=splat)

            a1, a2 = event_ms(fuse_gt), event_ms(tail_fuse)
            b1, b2 = event_ms(fuse_gt), event_ms(tail_fuse)
            torch.cuda.synchronize()
            st = buf.stats.cpu().numpy()
            ta, tb, tt = statistics.median([a1[0], b1[0]]), statistics.median([a2[0], b2[0]]), statistics.median([t[0] for t in t_tail])
            out["C%d_splat%d" % (C, splat)] = {
                "clouds": S, "fuse_ms": round(ta, 4), "fuse_ms_regions": [round(v, 4) for v in a1[1] + b1[1]], "tail_ms": round(tt, 4),
                "tail_ms_regions": [round(v, 4) for t in t_tail for v in t[1]], "tail_fuse_ms": round(tb, 4),
                "tail_fuse_ms_regions": [round(v, 4) for v in a2[1] + b2[1]], "fuse_behind_tail_ms": round(tb - tt, 4),
                "tail_success": int(tail[2][:, 0].sum()), "in_picture_per_image": int(st[:, 0].mean()), "visible_per_image": int(st[:, 1].mean()),
                "pixels_hit_per_image": int(st[:, 2].mean()), "atomics_per_submission": int(st[:, 0].sum()) * (2 * splat + 1) ** 2}
    return out


def git_state():
    try:
        head = subprocess.check_output(["git", "rev-parse", "HEAD"], cwd=ROOT, stderr=subprocess.DEVNULL).decode().strip()
        dirty = bool(subprocess.check_output(["git", "status", "--porcelain"], cwd=ROOT, stderr=subprocess.DEVNULL).strip())
        return {"based_on": head, "tree_differs": dirty}
    except Exception:
        return {"based_on": None, "tree_differs": None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fusion.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fuse_bench needs a GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    rec = {"tool": "tools/fuse_bench.py", "device": torch.cuda.get_device_name(0), "images": F, "points_per_cloud": N, "image": [H, W],
           "pose_iterations": ITERS, "timing": "HIP events, median of 9 regions of 20 calls after 5 warm-up calls, each form measured twice, alternated",
           "bytes_estimate_per_submission": F * H * W * (8 + 8 + 4 + 4) + F * N * (12 + 1) + F * N * 16, "by_cameras_and_splat": measure(dev)}
    rec.update(git_state())
    line = json.dumps(rec)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
