#!/usr/bin/env python
"""GPU tool: every KPConv aggregation launch of one stack-mode submission alone on the chip (hipGraph of 20 back-to-back replays, HIP
events), on the neighbour tables of a synthetic pyramid and random features of each layer's width, in the form the forward uses
(bf16 planes from 4 frames per submission, the stage's processing order); and, per layer, how many of the 128 neighbours of a query lie
inside the kernel's support max|kp| + sigma (`nin`: mean / p95 / max, computed on the host from the tables), and the share of queries
whose record gather reads 1 / 2 / 3 chunks (neighbours 0 - 15, 16 - 63, 64 - 127) in the sorted form - the fp32 emulation of the
kernels' stop rule that the CPU test uses (tests/kpconv_prefix_ref.py), on frame 0's tables.
    python tools/kpconv_probe.py [frames=16] [points=20480]      -> a markdown table on stdout
COFI_KPCONV_RECORDS=0 times the staging from separate position / flag arrays, COFI_KPCONV_PREFIX=0 the unsorted kernels (the launch
that writes the flag bits of the sorted form is part of the layer's time)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np
import torch

import kpconv_prefix_ref as prefix_ref
from tools.gemm_shapes import time_graph


def kernel_form(C):
    if C <= 4:
        return "c4"
    if C in (256, 512):
        return "shared<%d>" % (C // 128)
    if C % 4 == 0 and C >= 64:
        return "<4,%d>" % (2 if C % 128 == 0 else 1)
    return "<2,1>" if C % 2 == 0 and C >= 32 else "<1,1>"


def main():
    from cofii2p_amd import kpfpn, ops, spec
    from cofii2p_amd.network import CoFiI2P
    from cofii2p_amd.preprocess import build_pyramid
    from cofii2p_amd.synth import make_frame, subsample_indices
    from cofii2p_amd.weights import kernel_point_table

    frames = int(sys.argv[1]) if len(sys.argv) > 1 else 16
    points = int(sys.argv[2]) if len(sys.argv) > 2 else 20480
    dev = torch.device("cuda", 0)
    pyrs = []
    for fid in range(frames):
        fr = make_frame(fid, points)
        sub = [torch.from_numpy(s).to(dev) for s in subsample_indices(points, 5, seed=1000 + fid)]
        pyr = build_pyramid(torch.from_numpy(fr.points).to(dev), sub)
        pyr["feats"] = torch.from_numpy(fr.feats).to(dev)
        pyrs.append(pyr)
    data = CoFiI2P.stack_frames(pyrs, [torch.zeros(1, 3, 8, 8, device=dev)] * frames)[0]
    pts, order = data["points"], data.get("order")
    srt = bool(data.get("sorted_tables"))
    g = torch.Generator().manual_seed(1)
    records = ops.kpconv_records()
    planes = frames >= kpfpn.AGG_PLANES_MIN_FRAMES
    print("| layer (%d frames of %d points, records %s, sorted form %s) | kernel | queries | C | nin mean / p95 / max | real steps (mean) | "
          "1 / 2 / 3 chunks | us |" % (frames, points, "on" if records else "off", "on" if srt and records and ops.kpconv_prefix() else "off"))
    print("|---|---|---|---|---|---|---|---|")
    total = 0.0
    with torch.no_grad(), ops.arithmetic("bf16x6"):
        for blk in spec.ENCODER:
            st = blk.stage
            q, s, idx = (pts[st], pts[st - 1], data["subsampling"][st - 1]) if blk.strided else (pts[st], pts[st], data["neighbors"][st])
            C = blk.cin if blk.kind == "conv" else blk.mid
            kp = torch.from_numpy(np.asarray(kernel_point_table(15, blk.radius), dtype=np.float32)).to(dev)
            rsup = float(kp.norm(dim=1).max()) + blk.sigma
            # nin on the host: frame 0's table (the frames are alike)
            Mf, Nf = q.shape[0] // frames, s.shape[0] // frames
            i0 = idx[:Mf].long().cpu()
            sp = torch.cat([s[:Nf].cpu().double(), torch.full((1, 3), 1e9, dtype=torch.float64)], 0)
            d = (sp[i0.clamp(0, Nf)] - q[:Mf].cpu().double()[:, None]).norm(dim=2)
            nin = ((d < rsup) & (i0 < Nf)).sum(1).double()
            # chunks of the sorted form's record gather, on the host
            i0n = i0.numpy()
            nvalid = (i0n < Nf).sum(1)
            s0 = np.concatenate([s[:Nf].cpu().numpy(), np.zeros((1, 3), dtype=np.float32)])[np.clip(i0n, 0, Nf)]
            ch = prefix_ref.chunks(q[:Mf].cpu().numpy(), s0, nvalid, prefix_ref.support_radius2(kp.cpu().numpy(), blk.sigma))
            share = [float((ch == c).mean()) for c in (1, 2, 3)]
            feats = torch.randn(s.shape[0], C, generator=g).to(dev)
            o = None if order is None else order[st]
            pl = planes and C > 4
            if C > 4 and records:   # in the forward the records arrive from the GroupNorm apply that produced feats
                feats.cofi_kp_records = (ops.kp_pack_support(feats, s), s.data_ptr())
            elif C > 4:
                feats.cofi_row_pos = ops.row_sum_positive(feats)
            t = time_graph(lambda: ops.kpconv_aggregate(feats, q, s, idx, kp, blk.sigma, frames=frames, order=o, planes=pl,
                                                        sorted_tables=srt and C <= kpfpn.PREFIX_MAX_CHANNELS))   # as kpfpn.run_fpn routes it
            total += t
            print("| %s | %s | %d | %d | %.1f / %.0f / %.0f | %.2f | %.3f / %.3f / %.3f | %.1f |"
                  % (blk.name, kernel_form(C), q.shape[0], C, float(nin.mean()), float(nin.quantile(0.95)), float(nin.max()),
                     float(torch.ceil(nin / 4).mean()), share[0], share[1], share[2], t * 1e6))
            del feats
    print("| **all 14 layers** | | | | | | | **%.1f** |" % (total * 1e6))


if __name__ == "__main__":
    main()
