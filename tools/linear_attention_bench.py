#!/usr/bin/env python
"""Softmax attention against linear attention, per call and per forward.  GPU tool:

    python tools/linear_attention_bench.py [--out profiles/linear_attention.json] [--no-forward]

HIP-event times after warm-up, median of repeated regions, the two forms alternated in one process (tools/rig_pose_bench.py:event_ms):
  calls     per (L, S, frames): softmax_ms = ops.attention (attention_parts + merge -> the plain matrix, the arithmetic of --arith),
            linear_ms = ops.linear_attention (summary + fold + apply, fp32 FMA); q / k / v are column slices of a (rows, 384) projection
            buffer, q_colscale explicit.  linear_GBps = the bytes the operator has to move (q, k, v read once, out written once) over
            linear_ms - its bound is the K / V and Q / O streams, not arithmetic.
  forward   frames/s of a hipGraph-replayed forward(mode='test') loop, one frame at a time, at the KITTI shape (160 x 512, 20 480 points)
            and the stress shape (896 x 1600, 40 960 points), one model per attention kind.
No threshold: the figures are what was measured.  One JSON line, also written to --out."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch

from cofii2p_amd import ops
from rig_pose_bench import event_ms

CALLS = [(1280, 1280, 1), (22400, 22400, 1), (22400, 2560, 1), (2560, 22400, 1), (1280, 1280, 16)]   # (L, S, frames); the last: the KITTI pair at 16 frames


def call_times(dev, arith):
    out = []
    g = torch.Generator().manual_seed(0)
    for L, S, F in CALLS:
        qb = (torch.randn(F * L, 384, generator=g) * 0.5).to(dev)
        kb = torch.randn(F * S, 384, generator=g).to(dev)
        q, k, v = qb[:, :128], kb[:, 128:256], kb[:, 256:]
        cs = torch.stack([ops.col_inv_norm(q[f * L:(f + 1) * L]) for f in range(F)])
        o_soft, o_lin = torch.empty((F * L, 128), device=dev), torch.empty((F * L, 128), device=dev)

        def softmax():
            with ops.arithmetic(arith):
                ops.attention(q, k, v, q_colscale=cs, frames=F, out=o_soft)

        def linear():
            ops.linear_attention(q, k, v, q_colscale=cs, frames=F, out=o_lin)

        calls = 20 if L * S * F <= 1280 * 1280 * 16 else 5
        fns = {"softmax_ms": softmax, "linear_ms": linear}
        first = {n: event_ms(fn, calls=calls) for n, fn in fns.items()}     # alternated: what shares the machine moves both
        second = {n: event_ms(fn, calls=calls) for n, fn in fns.items()}
        rec = {"L": L, "S": S, "frames": F}
        for n in fns:
            rec[n] = round(statistics.median([first[n][0], second[n][0]]), 5)
            rec[n + "_regions"] = [round(t, 5) for t in first[n][1] + second[n][1]]
        nbytes = 4 * 128 * F * (2 * L + 2 * S)
        rec["linear_bytes"] = nbytes
        rec["linear_GBps"] = round(nbytes / (rec["linear_ms"] * 1e-3) / 1e9, 2)
        rec["softmax_over_linear"] = round(rec["softmax_ms"] / rec["linear_ms"], 3)
        out.append(rec)
    return out


def forward_rates(dev, arith):
    from cofii2p_amd.network import CoFiI2P
    from cofii2p_amd.preprocess import build_pyramid
    from cofii2p_amd.synth import make_frame, subsample_indices

    out = {}
    for name, (H, W, npts, steps) in (("kitti", (160, 512, 20480, 100)), ("stress", (896, 1600, 40960, 10))):
        class Opt:
            img_H, img_W, img_fine_resolution_scale, norm = H, W, 32, "gn"

        fr = make_frame(0, num_points=npts, img_hw=(H, W))
        sub = [torch.from_numpy(s).to(dev) for s in subsample_indices(npts, 5, seed=1000)]
        pyr = build_pyramid(torch.from_numpy(fr.points).to(dev), sub)
        pyr["feats"] = torch.from_numpy(fr.feats).to(dev)
        img = torch.from_numpy(fr.img)[None].to(dev)
        models = {}
        for kind in ("full", "linear"):
            m = CoFiI2P(Opt(), arithmetic=arith, attention=kind).to(dev)
            m.enable_graphs(True)
            for _ in range(3):
                m(pyr, img, None, None, None, "test")
            models[kind] = m
        rec = {"image": [H, W], "points": npts, "steps_per_region": steps}
        rates = {kind: [] for kind in models}
        for _ in range(3):                       # regions alternate between the two kinds
            for kind, m in models.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(steps):
                    res = m(pyr, img, None, None, None, "test")
                torch.cuda.synchronize()
                rates[kind].append(steps / (time.perf_counter() - t0))
                rec["matches_" + kind] = int(res[6].shape[1])
        for kind in models:
            rec["frames_per_s_" + kind] = round(statistics.median(rates[kind]), 2)
            rec["frames_per_s_%s_regions" % kind] = [round(r, 2) for r in rates[kind]]
        out[name] = rec
        del models
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "linear_attention.json"))
    ap.add_argument("--arith", default="bf16x6", choices=["f32", "bf16x3", "bf16x6"], help="arithmetic of the softmax kernel and of the forward's contractions")
    ap.add_argument("--no-forward", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("linear_attention_bench needs a GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    rec = {"tool": "tools/linear_attention_bench.py", "device": torch.cuda.get_device_name(0), "arithmetic": args.arith,
           "timing": "calls: HIP events, median of 9 regions of 20 (5 for the large shapes) calls after 5 warm-up calls, the forms alternated twice; "
                     "forward: host clock around graph-replayed forwards ending in a synchronise, median of 3 alternated regions"}
    rec["calls"] = call_times(dev, args.arith)
    if not args.no_forward:
        rec["forward"] = forward_rates(dev, args.arith)
    line = json.dumps(rec)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
