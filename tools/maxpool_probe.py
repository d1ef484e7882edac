#!/usr/bin/env python
"""GPU tool: the neighbour max-pool of the four strided residual blocks of one stack-mode submission, each alone on the chip (hipGraph
of 20 back-to-back launches, HIP events around a replay), at the forward's own shapes - the pyramid of bench.make_inputs, stacked as the
bench stacks it, random features of the block's input width, the stage's processing order - on the gather kernel
(cofi_neighbor_maxpool) and on the slice kernel (cofi_neighbor_maxpool_slice), three runs each, alternating.
    python tools/maxpool_probe.py [batch=16] [points=20480]      -> a markdown table on stdout
`routed`: whether ops.neighbor_maxpool sends the block to the slice kernel at this batch (ops.MAXPOOL_SLICE_MIN_FRAMES,
ops.MAXPOOL_SLICE_MAX_ROWS, COFI_MAXPOOL_SLICE)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bench
from tools.gemm_shapes import time_graph


def main():
    from cofii2p_amd import _lib, ops, spec
    from cofii2p_amd.network import CoFiI2P

    frames = int(sys.argv[1]) if len(sys.argv) > 1 else 16
    points = int(sys.argv[2]) if len(sys.argv) > 2 else 20480
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    made = bench.make_inputs(dev, list(range(frames)), points)
    data = CoFiI2P.stack_frames([f[0] for f in made], [f[1] for f in made])[0]
    order = data.get("order")
    g = torch.Generator().manual_seed(1)
    print("| block (%d frames of %d points) | source rows / frame | queries / frame | channels | H | gather kernel us (3 runs) | "
          "slice kernel us (3 runs) | new / old (medians) | routed |" % (frames, points))
    print("|---|---|---|---|---|---|---|---|---|")
    with torch.no_grad():
        for blk in spec.ENCODER:
            if not blk.strided:
                continue
            idx = data["subsampling"][blk.stage - 1]
            N, M, H, C = data["points"][blk.stage - 1].shape[0] // frames, idx.shape[0] // frames, idx.shape[1], blk.cin
            x = torch.randn(frames * N, C, generator=g).to(dev)
            o = None if order is None else order[blk.stage]
            out = torch.empty((frames * M, C), dtype=torch.float32, device=dev)

            def old():
                _lib.check(lib.cofi_neighbor_maxpool(ops._p(x), C, N, C, ops._p(idx), M, H, ops._p(out), C, frames, ops._p(o), ops._stream()),
                           "cofi_neighbor_maxpool")

            fits = ops.neighbor_maxpool_slice_ok(N, C, H, frames)
            told, tnew = [], []
            for _ in range(3):
                told.append(time_graph(old) * 1e6)
                if fits:
                    tnew.append(time_graph(lambda: ops.neighbor_maxpool_slice(x, idx, out=out, frames=frames, order=o)) * 1e6)
            if fits:   # the same bits, while we are here
                a = out.clone()
                old()
                assert torch.equal(a, out), blk.name
            routed = fits and frames >= ops.MAXPOOL_SLICE_MIN_FRAMES and N <= ops.MAXPOOL_SLICE_MAX_ROWS and ops.maxpool_slice()
            print("| %s | %d | %d | %d | %d | %s | %s | %s | %s |"
                  % (blk.name, N, M, C, H, " / ".join("%.1f" % t for t in told), " / ".join("%.1f" % t for t in tnew) if fits else "does not fit",
                     "%.3f" % (sorted(tnew)[1] / sorted(told)[1]) if fits else "-", "yes" if routed else "no"))
            del x, out


if __name__ == "__main__":
    main()
