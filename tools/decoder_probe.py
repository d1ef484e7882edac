#!/usr/bin/env python
"""GPU tool: the launches of the three FPN decoders in both forms, one launch at a time (hipGraph of 20 back-to-back replays, HIP
events), on random operands of the forward's shapes in the flagship arithmetic (bf16x6 + f16x3, static weights pre-split):
  concat form:     cofi_gather_rows into [up | stage], one GEMM over the whole buffer
  projected form:  GEMM over the coarse rows, then the skip GEMM with the indexed residual
    python tools/decoder_probe.py [frames=16] [points=20480]      -> a markdown table on stdout"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from tools.gemm_shapes import time_graph


def main():
    from cofii2p_amd import ops

    frames = int(sys.argv[1]) if len(sys.argv) > 1 else 16
    points = int(sys.argv[2]) if len(sys.argv) > 2 else 20480
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(1)
    print("| decoder (%d frames of %d points) | launch | M x N x K | us |" % (frames, points))
    print("|---|---|---|---|")
    with torch.no_grad(), ops.arithmetic("bf16x6"):
        for name, stage, cout, up, cin in (("decoder4", 3, 1024, 2048, 3072), ("decoder3", 2, 512, 1024, 1536), ("decoder2", 1, 64, 512, 768)):
            rows, crow = points >> stage, points >> (stage + 1)
            M, Mc = rows * frames, crow * frames
            w = torch.randn(cout, cin, generator=g) / cin ** 0.5
            W, Wu, Ws = (ops.presplit(t.contiguous().to(dev)) for t in (w, w[:, :up], w[:, up:]))
            bias = torch.randn(cout, generator=g).to(dev)
            coarse = torch.randn(Mc, up, generator=g).to(dev)
            cat = torch.randn(M, cin, generator=g).to(dev)
            stage_x = cat[:, up:].contiguous()
            idx = torch.randint(0, crow, (M, 1), generator=g, dtype=torch.int32).to(dev)
            sw = cout // 32 if name != "decoder2" else 0
            l2 = name == "decoder2"

            def dense(a, wt, **kw):
                if sw:
                    return ops.gemm_colstats(a, wt, stat_width=sw, frames=frames, **kw)
                return ops.gemm(a, wt, frames=frames, l2norm=l2 and "bias" in kw, **kw)

            proj = ops.gemm(coarse, Wu, frames=frames)
            t_gather = time_graph(lambda: ops.gather_rows(coarse, idx, out=cat[:, :up], frames=frames))
            t_cat = time_graph(lambda: dense(cat, W, bias=bias))
            t_proj = time_graph(lambda: ops.gemm(coarse, Wu, frames=frames))
            t_skip = time_graph(lambda: dense(stage_x, Ws, bias=bias, res=proj, res_idx=idx))
            t_skip0 = time_graph(lambda: dense(stage_x, Ws, bias=bias))
            for what, shape, t in (("concat: gather_rows", "%d x %d" % (M, up), t_gather), ("concat: GEMM", "%d x %d x %d" % (M, cout, cin), t_cat),
                                   ("projected: coarse GEMM", "%d x %d x %d" % (Mc, cout, up), t_proj),
                                   ("projected: skip GEMM + indexed residual", "%d x %d x %d" % (M, cout, cin - up), t_skip),
                                   ("(skip GEMM without the residual)", "%d x %d x %d" % (M, cout, cin - up), t_skip0)):
                print("| %s | %s | %s | %.1f |" % (name, what, shape, t * 1e6))
            print("| %s | **concat total / projected total** | | **%.1f / %.1f** |" % (name, (t_gather + t_cat) * 1e6, (t_proj + t_skip) * 1e6))
            del cat, coarse, stage_x, proj


if __name__ == "__main__":
    main()
