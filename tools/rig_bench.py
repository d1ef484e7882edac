#!/usr/bin/env python
"""What a rig submission saves: B = 16 images over S clouds in one forward (forward_async(..., cameras=C)) against the replicated-cloud
stack of 16 frames that serves the same images without the feature.  GPU tool:

    python tools/rig_bench.py [--out profiles/rig_mode.json] [--no-pyramid]

KITTI shape (20480 points, 160 x 512 images), bf16x6, hipGraphs, inputs read in place, four submissions in flight on
`frame_streams(4)`.  (S, C) = (16,1), (8,2), (4,4), (2,8); (16,1) is the same call in both forms - the noise floor of the comparison.
For every shape the two forms ALTERNATE in one process: a region is `--subs` submissions round-robin over the four streams, timed with
HIP events (start: all streams idle; stop: a stream that waits for the four), median of `--regions` regions per form -> images/s.
  forward       the forward alone, both forms on inputs that already sit in HBM
  with_pyramid  preprocess.PyramidGraph (upsample_k=1) in front, on the submission's stream: the rig builds S pyramids per submission
                and copies each into the stack once (FrameStack.put_cloud), the replicated form builds one per IMAGE, as it must today
                (FrameStack.put) - 16 builds of C-fold repeated clouds
One JSON line, also written to --out."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

B, POINTS, NSTREAMS = 16, 20480, 4
SHAPES = ((16, 1), (8, 2), (4, 4), (2, 8))


def timed_region(model, streams, submit, subs):
    """`subs` submissions, submission i on stream i % 4 in slot position i % 4 -> milliseconds between 'all idle' and 'all done'"""
    torch.cuda.synchronize()
    timer = streams[0]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(timer)
    for s in streams[1:]:
        s.wait_event(e0)
    pend = [None] * NSTREAMS
    for i in range(subs):
        k = i % NSTREAMS
        if pend[k] is not None:
            model.finish(pend[k], per_frame_errors=True)
        with torch.cuda.stream(streams[k]):
            pend[k] = submit(k)
    for s in streams[1:]:
        timer.wait_stream(s)
    e1.record(timer)
    for h in pend:
        if h is not None:
            model.finish(h, per_frame_errors=True)
    e1.synchronize()
    return e0.elapsed_time(e1)


def alternate(model, streams, forms, subs, regions, warm=2):
    """forms: {name: submit(k)}; the forms take turns region by region -> {name: {"images_per_s", "regions"}}"""
    for _ in range(warm):   # captures the graphs of these slots
        for submit in forms.values():
            timed_region(model, streams, submit, 2 * NSTREAMS)
    per = {name: [] for name in forms}
    for _ in range(regions):
        for name, submit in forms.items():
            per[name].append(subs * B / (1e-3 * timed_region(model, streams, submit, subs)))
    return {name: {"images_per_s": round(statistics.median(v), 1), "regions": [round(x, 1) for x in v]} for name, v in per.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rig_mode.json"))
    ap.add_argument("--subs", type=int, default=16, help="submissions per timed region")
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--no-pyramid", action="store_true", help="skip the rows with the KNN pyramid in front")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rig_bench needs a GPU: nothing is measured without one")
    import bench
    from cofii2p_amd.network import CoFiI2P
    from cofii2p_amd.preprocess import FrameStack, PyramidGraph
    from cofii2p_amd.synth import subsample_indices

    dev = torch.device("cuda", 0)
    model = CoFiI2P(bench.Opt(), arithmetic="bf16x6").to(dev)
    frames = bench.make_inputs(dev, list(range(B)), POINTS)
    pyrs, imgs = [f[0] for f in frames], [f[1] for f in frames]
    raw = [torch.from_numpy(f[2].points).to(dev) for f in frames]
    subs_idx = [[torch.from_numpy(s).to(dev) for s in subsample_indices(POINTS, 5, seed=1000 + i)] for i in range(B)]
    streams = model.frame_streams(NSTREAMS)
    rec = {"tool": "tools/rig_bench.py", "device": torch.cuda.get_device_name(0), "images_per_submission": B, "points": POINTS,
           "arithmetic": "bf16x6", "in_flight": NSTREAMS,
           "timing": "HIP events around %d submissions round-robin on 4 streams, forms alternating, median of %d regions per form" % (args.subs, args.regions),
           "forward": {}, "with_pyramid": {}}
    for si, (S, C) in enumerate(SHAPES):
        model.enable_graphs(False)   # drops the graphs (and their memory pools) of the previous shape
        torch.cuda.empty_cache()
        model.enable_graphs(True)
        tag = "S%d_C%d" % (S, C)
        rig, img = CoFiI2P.stack_frames(pyrs[:S], imgs)
        rep, _ = CoFiI2P.stack_frames([pyrs[f // C] for f in range(B)], imgs)
        forms = {"rig": lambda k: model.forward_async(300 + k, rig, img, inputs_stable=True, cameras=C),
                 "replicated": lambda k: model.forward_async(320 + k, rep, img, inputs_stable=True)}
        r = alternate(model, streams, forms, args.subs, args.regions)
        r["rig_over_replicated"] = round(r["rig"]["images_per_s"] / r["replicated"]["images_per_s"], 4)
        rec["forward"][tag] = r
        print(tag, "forward", json.dumps(r), file=sys.stderr, flush=True)
        del rig, rep, forms
        if args.no_pyramid:
            continue
        # the KNN pyramid in the chain: one PyramidGraph per stream, one static stack per slot and form, the images static
        sub_sizes = [int(t.shape[0]) for t in subs_idx[0]]
        pgs = [PyramidGraph(POINTS, sub_sizes, dev, capture_stream=streams[0], upsample_k=1) for _ in range(NSTREAMS)]
        tmpl = pgs[0].run(raw[0], subs_idx[0])
        feats = [p["feats"] for p in pyrs]
        st_rig = [FrameStack(tmpl, feats[0], imgs[0], B, cameras=C) for _ in range(NSTREAMS)]
        st_rep = [FrameStack(tmpl, feats[0], imgs[0], B) for _ in range(NSTREAMS)]

        def sub_rig(k):
            for s in range(S):
                st_rig[k].put_cloud(s, pgs[k].run(raw[s], subs_idx[s]), feats[s])
            for f in range(B):
                st_rig[k].put_image(f, imgs[f])
            return model.forward_async(340 + k, st_rig[k].pyr, st_rig[k].img, inputs_stable=True, cameras=C)

        def sub_rep(k):
            for f in range(B):
                st_rep[k].put(f, pgs[k].run(raw[f // C], subs_idx[f // C]), feats[f // C], imgs[f])
            return model.forward_async(360 + k, st_rep[k].pyr, st_rep[k].img, inputs_stable=True)

        r = alternate(model, streams, {"rig": sub_rig, "replicated": sub_rep}, args.subs, args.regions)
        r["rig_over_replicated"] = round(r["rig"]["images_per_s"] / r["replicated"]["images_per_s"], 4)
        rec["with_pyramid"][tag] = r
        print(tag, "with_pyramid", json.dumps(r), file=sys.stderr, flush=True)
        del pgs, st_rig, st_rep, sub_rig, sub_rep
    line = json.dumps(rec)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
