#!/usr/bin/env python
"""Time of the surface-normal estimation of a raw scan (cofii2p_amd/normals.py, csrc/normals.hip), GPU tool:

    python tools/normals_bench.py [--points 120000] [--k 30] [--out profiles/normals.json]

Three items on synth.make_raw_scan(num_points=...), each the median of repeated timed regions (a region = several calls on one stream,
closed by a device synchronise, host clock; warmed up first):
  (a) the k-nearest grid build plus the k = 30 self search in cell order (ops.KnnGrid + search),
  (b) the estimator kernel alone on those rows (cofi_estimate_normals),
  (c) FramePreparer.begin() + complete() of the frame with normals='given' ((7, N) scan) against normals='estimate' ((4, N) scan),
      regions of the two alternating in one process.
Writes one JSON file with the three times, the commit hash and whether the measured tree differed from that commit."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from cofii2p_amd import dataside, normals, ops, synth


def region_ms(fn, calls):
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / calls


def median_ms(fn, calls=10, regions=7, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t = [region_ms(fn, calls) for _ in range(regions)]
    return {"median_ms": round(statistics.median(t), 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4)}


def tree_state():
    """-> (hash of HEAD, True when the measured tree differs from it); (None, None) outside a git checkout"""
    try:
        head = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
        dirty = bool(subprocess.run(["git", "-C", ROOT, "status", "--porcelain"], capture_output=True, text=True, check=True).stdout.strip())
        return head, dirty
    except Exception:
        return None, None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=120000)
    ap.add_argument("--k", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "normals.json"))
    ap.add_argument("--commit", default=None, help="hash of the commit the tree was checked out from, for a tree that is no git checkout")
    ap.add_argument("--dirty", action="store_true", help="with --commit: the measured tree differs from that commit")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    opt = types.SimpleNamespace(img_H=160, img_W=512, num_pc=20480, num_kpt=64, P_tx_amplitude=10, P_ty_amplitude=0, P_tz_amplitude=10,
                                P_Rx_amplitude=0.0, P_Ry_amplitude=2 * np.pi, P_Rz_amplitude=0.0)
    raw, img, K = synth.make_raw_scan(0, num_points=args.points)
    cal = dataside.calib_matrices(synth.KITTI_CALIB_LINES)
    P_Tr = np.dot(cal["P2"], cal["Tr"])
    raw7, raw4, img_d = torch.from_numpy(raw).to(dev), torch.from_numpy(np.ascontiguousarray(raw[:4])).to(dev), torch.from_numpy(img).to(dev)
    pts = raw7[:3].t().contiguous()
    N = pts.shape[0]

    def search():
        g = ops.KnnGrid(pts)
        return g.search(pts, args.k, qorder=g.order), None   # no radius: no distance table, as estimate_normals searches

    head, dirty = (args.commit, args.dirty) if args.commit else tree_state()
    res = {"tool": "tools/normals_bench.py", "commit": head, "tree_differs_from_commit": dirty, "device": torch.cuda.get_device_name(0), "points": N, "k": args.k,
           "method": "median of 7 timed regions of 10 calls (host clock around work that ends in a device synchronise), 3 warm-up calls"}
    res["grid_build_and_self_search"] = median_ms(search)
    idx, _ = search()
    out = torch.empty((N, 3), dtype=torch.float32, device=dev)
    res["estimator_kernel"] = median_ms(lambda: normals.normals_from_rows(pts, idx, None, out=out))
    res["estimate_normals_end_to_end"] = median_ms(lambda: normals.estimate_normals(pts, k=args.k, out=out))
    _, degenerate = normals.estimate_normals(pts, k=args.k, return_degenerate=True)
    res["degenerate_rows"] = degenerate

    preps = {"given": (dataside.FramePreparer(opt, dev), raw7), "estimate": (dataside.FramePreparer(opt, dev, normals="estimate", normals_k=args.k), raw4)}

    def frame(which):
        prep, scan = preps[which]
        return lambda: prep.complete(prep.begin(scan, img_d, K, P_Tr, 0))

    for which in preps:
        for _ in range(3):
            frame(which)()
    torch.cuda.synchronize()
    t = {"given": [], "estimate": []}
    for _ in range(7):
        for which in preps:          # alternating regions: both forms see the same machine state
            t[which].append(region_ms(frame(which), 5))
    for which in preps:
        res["prepare_" + which] = {"median_ms": round(statistics.median(t[which]), 4), "min_ms": round(min(t[which]), 4), "max_ms": round(max(t[which]), 4)}
    res["prepare_estimate_minus_given_ms"] = round(res["prepare_estimate"]["median_ms"] - res["prepare_given"]["median_ms"], 4)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
