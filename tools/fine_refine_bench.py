#!/usr/bin/env python
"""What sub-pixel fine matches cost: forward_async(pose_K=K) with and without subpixel=True, in the configuration bench.py measures.
GPU tool, three steps:

    python tools/fine_refine_bench.py [--out profiles/fine_refine.json]            # 1. frames/s, flag off and on alternated
    rocprofv3 --kernel-trace -d DIR -o x -- python tools/fine_refine_bench.py --trace-target       # 2. a run of its own for the trace
    python tools/fine_refine_bench.py --merge-trace DIR/.../x_results.db [--out ...]               # 3. the launch's own time -> the JSON

Step 1: KITTI shape (20480 points, 160 x 512 images), bf16x6, hipGraphs, inputs read in place, 16 frames per submission, four
submissions in flight on `frame_streams(4)`, 10 000 pose hypotheses per frame behind every forward.  The two forms ALTERNATE in one
process: a region is `--subs` submissions round-robin over the four streams, timed with HIP events (start: all streams idle; stop: a
stream that waits for the four), median of `--regions` regions per form -> frames/s, with every region on record.
Step 2 submits `--subs` stacks with the flag on, on one stream, under the profiler; step 3 reads the durations of fine_refine_kernel (and,
for scale, of match_finish_kernel in front of it) from the trace's `kernels` table.  No figure is fixed in advance."""
import argparse
import json
import os
import sqlite3
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

B, POINTS, NSTREAMS, ITERS = 16, 20480, 4, 10000


def merge_trace(db, out):
    cur = sqlite3.connect(db).cursor()
    cols = [r[1] for r in cur.execute("pragma table_info(kernels)")]
    name_col = "name" if "name" in cols else [c for c in cols if "name" in c][0]
    rec = {}
    for key in ("fine_refine_kernel", "match_finish_kernel"):
        us = [(e - s) / 1e3 for s, e in cur.execute("select start, end from kernels where %s like ? order by start" % name_col, ("%" + key + "%",))]
        if not us:
            raise SystemExit("no dispatch of %s in %s" % (key, db))
        us = us[len(us) // 4:]   # the first quarter: warm-up and capture runs
        rec[key] = {"dispatches": len(us), "median_us": round(statistics.median(us), 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2)}
    data = json.load(open(out)) if os.path.exists(out) else {"tool": "tools/fine_refine_bench.py"}
    data["kernel_trace"] = dict(rec, source="rocprofv3 --kernel-trace of --trace-target: %d frames per dispatch, one stream, flag on" % B)
    with open(out, "w") as fh:
        fh.write(json.dumps(data) + "\n")
    print(json.dumps(data["kernel_trace"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fine_refine.json"))
    ap.add_argument("--subs", type=int, default=16, help="submissions per timed region")
    ap.add_argument("--regions", type=int, default=9)
    ap.add_argument("--trace-target", action="store_true", help="submit --subs stacks with the flag on and leave: the run a kernel trace is taken of")
    ap.add_argument("--merge-trace", metavar="DB", default=None, help="rocpd database of such a run: its kernel durations go into --out (no GPU needed)")
    args = ap.parse_args()
    if args.merge_trace:
        return merge_trace(args.merge_trace, args.out)
    import numpy as np
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("fine_refine_bench needs a GPU: nothing is measured without one")
    import bench
    from cofii2p_amd.network import CoFiI2P
    from rig_bench import alternate

    dev = torch.device("cuda", 0)
    model = CoFiI2P(bench.Opt(), arithmetic="bf16x6").to(dev)
    frames = bench.make_inputs(dev, list(range(B)), POINTS)
    stacked, imgs = CoFiI2P.stack_frames([f[0] for f in frames], [f[1] for f in frames])
    K = torch.from_numpy(np.stack([np.array([[300.0 + 4 * f, 0, 128.0], [0, 296.0 + 2 * f, 40.0], [0, 0, 1.0]]) for f in range(B)]).astype(np.float32)).to(dev)
    model.enable_graphs(True)
    if args.trace_target:
        for _ in range(args.subs):
            model.finish(model.forward_async(400, stacked, imgs, inputs_stable=True, pose_K=K, pose_iterations=ITERS, subpixel=True),
                         per_frame_errors=True)
        torch.cuda.synchronize()
        return
    streams = model.frame_streams(NSTREAMS)
    forms = {"off": lambda k: model.forward_async(400 + k, stacked, imgs, inputs_stable=True, pose_K=K, pose_iterations=ITERS),
             "on": lambda k: model.forward_async(420 + k, stacked, imgs, inputs_stable=True, pose_K=K, pose_iterations=ITERS, subpixel=True)}
    r = alternate(model, streams, forms, args.subs, args.regions)
    rec = {"tool": "tools/fine_refine_bench.py", "device": torch.cuda.get_device_name(0), "frames_per_submission": B, "points": POINTS,
           "arithmetic": "bf16x6", "in_flight": NSTREAMS, "pose_iterations": ITERS,
           "timing": "HIP events around %d submissions round-robin on 4 streams, flag off and on alternating, median of %d regions per form"
                     % (args.subs, args.regions)}
    for name, v in r.items():
        reg = v["regions"]
        rec[name] = {"frames_per_s": v["images_per_s"], "min": min(reg), "max": max(reg), "regions": reg}
    rec["on_over_off"] = round(rec["on"]["frames_per_s"] / rec["off"]["frames_per_s"], 4)
    h = model.forward_async(420, stacked, imgs, inputs_stable=True, pose_K=K, pose_iterations=ITERS, subpixel=True)
    model.finish(h, per_frame_errors=True)
    rec["matches_per_frame"] = [int(v) for v in h["count_host"][:, 0]]
    if os.path.exists(args.out):   # a kernel trace merged earlier stays
        old = json.load(open(args.out))
        if "kernel_trace" in old:
            rec["kernel_trace"] = old["kernel_trace"]
    line = json.dumps(rec)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
