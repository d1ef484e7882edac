#!/usr/bin/env python
"""What ONE pose per rig costs against the per-image batched tail it replaces, and what it buys on starved rigs.  GPU tool:

    python tools/rig_pose_bench.py [--out profiles/rig_pose.json] [--no-pipeline]

16 images of synthetic correspondences (~400 valid rows each in buffers of cap = 1280, 30 % outliers, 0.5 px noise; every camera's
points lie in front of that camera, the cameras spread around the rig's vertical axis about 0.5 m from it), 10 000 hypotheses, HIP-event
times after warm-up, median of repeated regions, the forms alternated in one process:
  (a) batched_16_ms   pose.solve_pnp_ransac_batch on the 16 images: 16 unrelated camera poses (the tail without rig_extrinsics)
  (b) rig_ms          pose.solve_pnp_ransac_rig on the SAME operands as S = 8 / 4 / 2 rigs of C = 2 / 4 / 8 cameras
frames/s of a serving.FrameBatcher loop (batch 16 = 4 rigs of 4 cameras, the bench's synthetic KITTI-shaped frames) with the pose off, the
per-image tail and the rig tail, and a table of starved rigs: success, RTE and RRE of (a) per image against (b).  One JSON line, also
written to --out."""
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

CAP, ITERS = 1280, 10000
W, H = 512.0, 160.0


def K4_of(c):
    return (700.0 + 8 * c, 700.0 - 4 * c, 256.0 + c, 80.0 - c)


def K_of(c):
    fx, fy, cx, cy = K4_of(c)
    return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])


def rot(axis, a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]) if axis == "y" else np.array([[1, 0, 0], [0, c, -s], [0, s, c]])


def extrinsics(C, rng):
    """(C,3,4) [R_c | t_c], camera <- rig: the cameras look outwards around the vertical (y) axis, about 0.5 m from it"""
    E = np.zeros((C, 3, 4))
    for c in range(C):
        yaw = 2 * np.pi * c / C + rng.uniform(-0.1, 0.1)
        Rc = rot("x", rng.uniform(-0.05, 0.05)) @ rot("y", -yaw)
        centre = 0.5 * np.array([np.sin(yaw), 0.0, np.cos(yaw)]) + rng.uniform(-0.05, 0.05, 3)
        E[c, :, :3], E[c, :, 3] = Rc, -Rc @ centre
    return E


def rig_scene(rng, counts, E, noise=0.5, outliers=0.3, inliers=None):
    """-> (Xs, uvs lists over the cameras, T = (R, t) ground truth rig <- cloud)"""
    w = rng.normal(size=3) * 0.4
    th = np.linalg.norm(w)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
    t = rng.normal(size=3) * 2
    Xs, uvs = [], []
    for c, n in enumerate(counts):
        fx, fy, cx, cy = K4_of(c)
        px = np.stack([rng.uniform(0, W, n), rng.uniform(0, H, n)], 1)
        depth = rng.uniform(6.0, 30.0, n)
        Yc = np.stack([(px[:, 0] - cx) / fx * depth, (px[:, 1] - cy) / fy * depth, depth], 1)
        X = ((Yc - E[c, :, 3]) @ E[c, :, :3] - t) @ R
        uv = px + rng.normal(size=(n, 2)) * noise
        n_out = n - inliers[c] if inliers is not None else int(round(outliers * n))
        out = rng.permutation(n)[:n_out]
        uv[out] = np.stack([rng.uniform(0, W, n_out), rng.uniform(0, H, n_out)], 1)
        Xs.append(X.astype(np.float32)), uvs.append(uv.astype(np.float32))
    return Xs, uvs, (R, t)


def pack(rigs, C, cap, dev):
    """rigs: list of (Xs, uvs, T) -> X (B,cap,3), fine_xy (B,2,cap) coordinate-major, K (B,3,3), counts (B,) on the device"""
    B = len(rigs) * C
    X, uv, counts = np.zeros((B, cap, 3), np.float32), np.zeros((B, cap, 2), np.float32), []
    for s, (Xs, uvs, _) in enumerate(rigs):
        for c in range(C):
            n = len(Xs[c])
            X[s * C + c, :n], uv[s * C + c, :n] = Xs[c], uvs[c]
            counts.append(n)
    Ks = np.stack([K_of(f % C) for f in range(B)]).astype(np.float32)
    return (torch.from_numpy(X).to(dev), torch.from_numpy(uv).to(dev).transpose(1, 2).contiguous(), torch.from_numpy(Ks).to(dev),
            torch.tensor(counts, dtype=torch.int32, device=dev))


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


def kernel_times(dev):
    out = {}
    for C in (2, 4, 8):
        S = 16 // C
        rng = np.random.default_rng(100 + C)
        E = extrinsics(C, rng)
        rigs = [rig_scene(rng, [int(rng.integers(360, 441)) for _ in range(C)], E) for _ in range(S)]
        X, fxy, Ks, cnt = pack(rigs, C, CAP, dev)
        ext = pose.rig_extrinsics(E, C, dev)
        B = S * C
        bufs_a = (torch.empty(pose.pnp_batch_workspace(ITERS, B), dtype=torch.uint8, device=dev), torch.empty((B, 12), device=dev),
                  torch.empty((B, 3), dtype=torch.int32, device=dev), torch.empty((B, CAP), dtype=torch.uint8, device=dev))
        bufs_b = (torch.empty(pose.pnp_rig_workspace(ITERS, S), dtype=torch.uint8, device=dev), torch.empty((S, 12), device=dev),
                  torch.empty((S, 3), dtype=torch.int32, device=dev)) + tuple(torch.empty_like(t) for t in bufs_a[1:])

        def a():
            pose.solve_pnp_ransac_batch_into(X, fxy, Ks, cnt, *bufs_a, iterations=ITERS, coord_major=True)

        def b():
            pose.solve_pnp_ransac_rig_into(X, fxy, Ks, ext, C, cnt, *bufs_b, iterations=ITERS, coord_major=True)

        ta1, ra1 = event_ms(a)      # alternated: what shares the box with this process moves both
        tb1, rb1 = event_ms(b)
        ta2, ra2 = event_ms(a)
        tb2, rb2 = event_ms(b)
        ta, tb = statistics.median([ta1, ta2]), statistics.median([tb1, tb2])
        torch.cuda.synchronize()
        errs = []
        for s, (_, _, T) in enumerate(rigs):
            P = np.eye(4)
            P[:3, :3], P[:3, 3] = bufs_b[1][s, :9].view(3, 3).cpu().numpy().astype(np.float64), bufs_b[1][s, 9:].cpu().numpy().astype(np.float64)
            G = np.eye(4)
            G[:3, :3], G[:3, 3] = T
            errs.append(pose.get_P_diff(P, G))
        out[str(C)] = {"rigs": S, "valid_rows": [int(c) for c in cnt.cpu()], "batched_16_ms": round(ta, 4),
                       "batched_16_ms_regions": [round(v, 4) for v in ra1 + ra2], "rig_ms": round(tb, 4),
                       "rig_ms_regions": [round(v, 4) for v in rb1 + rb2], "rig_over_batched": round(tb / ta, 4),
                       "rig_success": [int(v) for v in bufs_b[2][:, 0].cpu()], "rig_inliers": [int(v) for v in bufs_b[2][:, 1].cpu()],
                       "rig_rte_m_max": round(max(e[0] for e in errs), 5), "rig_rre_deg_max": round(max(e[1] for e in errs), 5)}
    return out


STARVED = {"40/2/3": ((40, 2, 3), (28, 2, 3)), "30/30/30": ((30, 30, 30), None), "12/9/3/20/0/7": ((12, 9, 3, 20, 0, 7), None),
           "5/6/4/5": ((5, 6, 4, 5), (3, 3, 3, 2))}


def starved_table(dev, iterations=512):
    """per-image poses of the batched tail against the one pose of the rig solve on rigs some of whose cameras are starved"""
    table = {}
    for i, (name, (counts, inl)) in enumerate(STARVED.items()):
        rng = np.random.default_rng(300 + i)
        C = len(counts)
        E = extrinsics(C, rng)
        Xs, uvs, T = rig_scene(rng, counts, E, inliers=inl)
        X, fxy, Ks, cnt = pack([(Xs, uvs, T)], C, 128, dev)
        res, R, t, _ = pose.solve_pnp_ransac_batch(X, fxy, Ks, count=cnt, iterations=iterations, coord_major=True)
        rig, per = pose.solve_pnp_ransac_rig(X, fxy, Ks, E, C, count=cnt, iterations=iterations, coord_major=True)
        torch.cuda.synchronize()
        G = np.eye(4)
        G[:3, :3], G[:3, 3] = T
        rows = []
        for c in range(C):
            Gc = np.eye(4)
            Gc[:3, :3], Gc[:3, 3] = E[c, :, :3] @ T[0], E[c, :, :3] @ T[1] + E[c, :, 3]
            ok = int(res[c, 0])
            e = pose.get_P_diff(pose.pose_matrix(R[c], t[c]), Gc) if ok else (None, None)
            rows.append({"rows": counts[c], "success": ok, "inliers": int(res[c, 1]), "rte_m": None if e[0] is None else round(float(e[0]), 5),
                         "rre_deg": None if e[1] is None else round(float(e[1]), 5)})
        ok = int(rig["result"][0, 0])
        e = pose.get_P_diff(pose.pose_matrix(rig["R"][0], rig["t"][0]), G) if ok else (None, None)
        table[name] = {"per_image": rows,
                       "rig": {"success": ok, "inliers": int(rig["result"][0, 1]), "inliers_per_image": [int(v) for v in per["result"][:, 1].cpu()],
                               "rte_m": None if e[0] is None else round(float(e[0]), 5), "rre_deg": None if e[1] is None else round(float(e[1]), 5)}}
    return table


def batcher_rates(dev, stacks=24, warm=10):
    """frames/s of a FrameBatcher loop over rigs of 4 cameras built from the bench's synthetic frames: pose off, per-image tail, rig tail"""
    import bench
    from cofii2p_amd.network import CoFiI2P
    from cofii2p_amd.serving import FrameBatcher

    B, C = 16, 4
    model = CoFiI2P(bench.Opt()).to(dev)
    model.enable_graphs(True)
    frames = bench.make_inputs(dev, list(range(B)), 20480)
    rigs = [(frames[s * C][0], torch.cat([frames[s * C + c][1] for c in range(C)])) for s in range(B // C)]
    Kd = torch.from_numpy(np.stack([np.array([[300.0, 0, 256.0], [0, 300.0, 80.0], [0, 0, 1.0]])] * C).astype(np.float32)).to(dev)
    E = extrinsics(C, np.random.default_rng(5))
    rates = {}
    for i, mode in enumerate(("off", "per_image", "rig")):
        fb = FrameBatcher(model, batch=B, cameras=C, slot_base=200 + 16 * i, pose=mode != "off", pose_iterations=ITERS,
                          rig_extrinsics=E if mode == "rig" else None)
        keep = []

        def consume(tickets):
            for tk in tickets:
                try:
                    fb.result(tk)
                except RuntimeError:
                    continue          # an image without matches
                if mode != "off":
                    keep.append(fb.pose_result(tk))
                if mode == "rig":
                    keep.append(fb.rig_pose_result(tk))
                del keep[:-4]

        def loop(n_stacks):
            pending = []
            for _ in range(n_stacks):
                pending.append([tk for pyr, imgs in rigs for tk in fb.submit_rig(pyr, imgs, K=Kd if mode != "off" else None)])
                if len(pending) > fb.ring - 2:
                    consume(pending.pop(0))
            while pending:
                consume(pending.pop(0))
            torch.cuda.synchronize()

        loop(warm)
        per = []
        for _ in range(3):
            t0 = time.perf_counter()
            loop(stacks)
            per.append(stacks * B / (time.perf_counter() - t0))
        rates[mode] = {"images_per_s": round(statistics.median(per), 1), "regions": [round(p, 1) for p in per]}
        fb.drain()
        del fb
    return rates


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rig_pose.json"))
    ap.add_argument("--no-pipeline", action="store_true", help="skip the FrameBatcher rates")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rig_pose_bench needs a GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    rec = {"tool": "tools/rig_pose_bench.py", "device": torch.cuda.get_device_name(0), "images": 16, "cap": CAP, "iterations": ITERS,
           "timing": "HIP events, median of 9 regions of 20 calls after 5 warm-up calls, (a) and (b) alternated twice",
           "by_cameras": kernel_times(dev), "starved_rigs_512_hypotheses": starved_table(dev)}
    if not args.no_pipeline:
        rec["frame_batcher_4_cameras"] = batcher_rates(dev)
    line = json.dumps(rec)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
