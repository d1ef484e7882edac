#!/usr/bin/env python
"""What the pose covariance costs next to the pose tail it follows.  GPU tool:

    python tools/pose_cov_bench.py [--out profiles/pose_cov.json]

The submission of tools/rig_pose_bench.py: 16 images of synthetic correspondences (~400 valid rows each in buffers of cap = 1280, 30 %
outliers, 0.5 px noise), 10 000 hypotheses.  HIP-event times after warm-up, median of repeated regions, the forms alternated in one
process:
  frame   (a) tail_ms  pose.solve_pnp_ransac_batch_into on the 16 images     (b) cov_ms  pose.pose_covariance_batch_into behind it
  rig     (a) tail_ms  pose.solve_pnp_ransac_rig_into, 4 rigs of 4 cameras   (b) cov_ms  pose.pose_covariance_rig_into behind it
          (c) cov_images_ms  the frame form on the 16 per-image poses, as forward_async(rig_extrinsics=, pose_cov=) adds it
The figure is cov_ms / tail_ms; there is no threshold.  One JSON line, also written to --out."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch

from cofii2p_amd import pose
from rig_pose_bench import CAP, ITERS, event_ms, extrinsics, pack, rig_scene


def measure(dev):
    C, S = 4, 4
    B = S * C
    rng = np.random.default_rng(104)
    E = extrinsics(C, rng)
    rigs = [rig_scene(rng, [int(rng.integers(360, 441)) for _ in range(C)], E) for _ in range(S)]
    X, fxy, Ks, cnt = pack(rigs, C, CAP, dev)
    ext = pose.rig_extrinsics(E, C, dev)
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)  # noqa: E731
    tail_f = (torch.empty(pose.pnp_batch_workspace(ITERS, B), dtype=torch.uint8, device=dev), torch.empty((B, 12), device=dev),
              torch.empty((B, 3), dtype=torch.int32, device=dev), torch.empty((B, CAP), dtype=torch.uint8, device=dev))
    tail_r = (torch.empty(pose.pnp_rig_workspace(ITERS, S), dtype=torch.uint8, device=dev), torch.empty((S, 12), device=dev),
              torch.empty((S, 3), dtype=torch.int32, device=dev)) + tuple(torch.empty_like(t) for t in tail_f[1:])
    cov_f, cov_r, cov_ri = (f64(B, 6, 6), f64(B, 6, 6), f64(B, 4)), (f64(S, 6, 6), f64(S, 6, 6), f64(S, 4)), (f64(B, 6, 6), f64(B, 6, 6), f64(B, 4))

    def frame_tail():
        pose.solve_pnp_ransac_batch_into(X, fxy, Ks, cnt, *tail_f, iterations=ITERS, coord_major=True)

    def frame_cov():
        pose.pose_covariance_batch_into(X, fxy, Ks, cnt, tail_f[1], tail_f[2], tail_f[3], *cov_f, coord_major=True)

    def rig_tail():
        pose.solve_pnp_ransac_rig_into(X, fxy, Ks, ext, C, cnt, *tail_r, iterations=ITERS, coord_major=True)

    def rig_cov():
        pose.pose_covariance_rig_into(X, fxy, Ks, ext, C, cnt, tail_r[1], tail_r[2], tail_r[5], *cov_r, coord_major=True)

    def rig_cov_images():
        pose.pose_covariance_batch_into(X, fxy, Ks, cnt, tail_r[3], tail_r[4], tail_r[5], *cov_ri, coord_major=True)

    out = {}
    for name, fns in (("frame", {"tail_ms": frame_tail, "cov_ms": frame_cov}),
                      ("rig", {"tail_ms": rig_tail, "cov_ms": rig_cov, "cov_images_ms": rig_cov_images})):
        first = {k: event_ms(fn) for k, fn in fns.items()}      # alternated: what shares the box with this process moves all of them
        second = {k: event_ms(fn) for k, fn in fns.items()}
        rec = {}
        for k in fns:
            rec[k] = round(statistics.median([first[k][0], second[k][0]]), 5)
            rec[k + "_regions"] = [round(v, 5) for v in first[k][1] + second[k][1]]
        rec["cov_over_tail"] = round(rec["cov_ms"] / rec["tail_ms"], 5)
        torch.cuda.synchronize()
        stat = (cov_f if name == "frame" else cov_r)[2]
        rec["bodies"], rec["ok"] = int(stat.shape[0]), int(stat[:, 0].sum())
        rec["rows_used"] = [int(v) for v in stat[:, 1].cpu()]
        cov = (cov_f if name == "frame" else cov_r)[0]
        rot, tra = pose.covariance_sigmas(cov)
        rec["rotation_sigma_deg"] = [round(float(v), 5) for v in rot.cpu()]
        rec["translation_sigma_m"] = [round(float(v), 5) for v in tra.cpu()]
        out[name] = rec
    out["valid_rows"] = [int(c) for c in cnt.cpu()]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_cov.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pose_cov_bench needs a GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    rec = {"tool": "tools/pose_cov_bench.py", "device": torch.cuda.get_device_name(0), "images": 16, "cap": CAP, "iterations": ITERS,
           "timing": "HIP events, median of 9 regions of 20 calls after 5 warm-up calls, the forms alternated twice"}
    rec.update(measure(dev))
    line = json.dumps(rec)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
