#!/usr/bin/env python
"""Time of the raw-sweep path (cofii2p_amd/sweeps.py, csrc/dataside.hip), GPU tool:

    python tools/sweeps_bench.py [--sweeps 7] [--points 34700] [--out profiles/sweeps.json]

On synth.make_raw_sweeps (7 sweeps x ~34 700 points, a 900 x 1600 image), each item the median of repeated timed regions (a region =
several calls on one stream, closed by a device synchronise, host clock; warmed up first):
  (a) the four stages alone on device-resident inputs, enqueue only (no wait on a count): accumulate (with the concatenation of the
      sweeps and the upload of offsets and matrices), float64 voxel grid, camera stage, image resize;
  (b) the public wrappers of the same stages, each with its pinned-copy-plus-event wait on the count it returns;
  (c) build_sample end to end from device-resident sweeps and images, and from host numpy arrays (uploads included);
  (d) the float32 voxel grid at the same point count: cofi_voxel_downsample at 0.2 m on the (N, 8) rows of the float32-rounded cloud
      (what the float64 keys and means cost over it), and FramePreparer.voxel_downsample as shipped (pack kernel + 0.1 m grid);
  (e) the numpy restatement (tests/sweeps_refs.py build_sample) on this machine's host, a few runs.
Writes one JSON file with the times, the counts of the sample, the commit hash and whether the measured tree differed from it."""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import sweeps_refs as R
from cofii2p_amd import _lib, dataside, sweeps, synth


def region_ms(fn, calls):
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / calls


def median_ms(fn, calls=50, regions=7, warm=3):
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
    ap.add_argument("--sweeps", type=int, default=7)
    ap.add_argument("--points", type=int, default=34700)
    ap.add_argument("--host-runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sweeps.json"))
    ap.add_argument("--commit", default=None, help="hash of the commit the tree was checked out from, for a tree that is no git checkout")
    ap.add_argument("--dirty", action="store_true", help="with --commit: the measured tree differs from that commit")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    s = synth.make_raw_sweeps(0, sweeps=args.sweeps, points_per_sweep=args.points)
    poses = [sweeps.pose_matrix(q, t) for q, t in s["ego_poses"]]
    calib = sweeps.pose_matrix(*s["lidar_calib"])
    Ts = sweeps.sweep_transforms(poses[0], poses[1:], calib)
    cams = [(c["img"], c["K"], sweeps.camera_from_lidar(poses[0], calib, sweeps.pose_matrix(*c["ego_pose"]), sweeps.pose_matrix(*c["calib"])))
            for c in s["cameras"]]
    sw_dev = [torch.from_numpy(x).to(dev) for x in s["sweeps"]]
    cams_dev = [(torch.from_numpy(img).to(dev), K, P) for img, K, P in cams]
    b = sweeps.SweepBuilder(dev)

    head, dirty = (args.commit, args.dirty) if args.commit else tree_state()
    res = {"tool": "tools/sweeps_bench.py", "commit": head, "tree_differs_from_commit": dirty, "device": torch.cuda.get_device_name(0),
           "sweeps": args.sweeps, "points_per_sweep": args.points, "image": list(cams[0][0].shape[:2]),
           "method": "median of 7 timed regions of 50 calls (host clock around work that ends in a device synchronise), 3 warm-up calls; "
                     "the two voxel grids in alternating regions"}
    sample = b.build_sample(sw_dev, Ts, cams_dev)
    if sample is None:
        raise SystemExit("the synthetic sample was rejected: %r" % (b.last,))
    res["sample"] = {k: sample[k] for k in ("accumulated", "voxels", "inside", "camera")}
    n, m = sample["accumulated"], sample["voxels"]

    # (a) stages, enqueue only
    pts, inten, _ = b._accumulate(sw_dev, Ts)
    pts, inten = pts[:n].clone(), inten[:n].clone()
    vox = b._voxel(pts, inten, sweeps.VOXEL_SIZE, None)[0][:m].clone()
    img0, K0, P0 = cams_dev[sample["camera"]]
    Ks = sweeps.scaled_intrinsics(K0)
    hw = sweeps.resized_hw(img0.shape[:2])
    st = {}
    st["accumulate"] = median_ms(lambda: b._accumulate(sw_dev, Ts))
    st["voxel_grid_f64"] = median_ms(lambda: b._voxel(pts, inten, sweeps.VOXEL_SIZE, None))
    st["to_camera"] = median_ms(lambda: b._camera(vox, P0, Ks, hw))
    st["resize_u8"] = median_ms(lambda: b.resize_u8(img0))
    res["stages_enqueue_only"] = st
    # (b) the public wrappers, each waiting on its count
    wr = {}
    wr["accumulate"] = median_ms(lambda: b.accumulate(sw_dev, Ts))
    wr["voxel_downsample"] = median_ms(lambda: b.voxel_downsample(pts, inten))
    wr["to_camera"] = median_ms(lambda: b.to_camera(vox, P0, Ks, hw))
    res["wrappers_with_count_wait"] = wr
    # (c) one sample end to end
    res["build_sample_device_inputs"] = median_ms(lambda: b.build_sample(sw_dev, Ts, cams_dev))
    res["build_sample_host_inputs"] = median_ms(lambda: b.build_sample(s["sweeps"], Ts, cams), calls=20)

    # (d) the float32 grid at the same point count
    lib = _lib.load()
    rows8 = torch.zeros((n, 8), dtype=torch.float32, device=dev)
    rows8[:, 0:3] = pts.to(torch.float32)
    rows8[:, 3] = inten
    out8 = torch.empty((n, 8), dtype=torch.float32, device=dev)
    cnt = torch.zeros(2, dtype=torch.int32, device=dev)
    ws = torch.empty(lib.cofi_voxel_downsample_workspace(n) + 256, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def f32_grid():
        _lib.check(lib.cofi_voxel_downsample(rows8.data_ptr(), n, sweeps.VOXEL_SIZE, out8.data_ptr(), n, cnt.data_ptr(), ws.data_ptr(), ws.numel(), stream),
                   "cofi_voxel_downsample")

    # alternating regions: both grids see the same machine state
    f64_grid = lambda: b._voxel(pts, inten, sweeps.VOXEL_SIZE, None)
    for fn in (f32_grid, f64_grid):
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    t = {"f32": [], "f64": []}
    for _ in range(7):
        t["f32"].append(region_ms(f32_grid, 50))
        t["f64"].append(region_ms(f64_grid, 50))
    res["voxel_grid_0p2_alternating"] = {k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
                                         for k, v in t.items()}
    res["voxel_grid_0p2_alternating"]["f32_voxels"] = int(cnt.cpu()[0])
    opt = types.SimpleNamespace(img_H=160, img_W=512, num_pc=20480, num_kpt=64)
    prep = dataside.FramePreparer(opt, dev)
    scan7 = torch.zeros((7, n), dtype=torch.float32, device=dev)
    scan7[0:3] = pts.to(torch.float32).t()
    scan7[3] = inten
    eye = torch.eye(4, dtype=torch.float32, device=dev)
    res["frame_preparer_voxel_downsample_0p1"] = median_ms(lambda: prep.voxel_downsample(scan7, eye))
    res["frame_preparer_voxel_downsample_0p1"]["voxels"] = prep.voxel_downsample(scan7, eye)[1]

    # (e) the numpy restatement on the host
    host = []
    for _ in range(args.host_runs):
        t0 = time.perf_counter()
        ref, why = R.build_sample(s["sweeps"], Ts, cams)
        host.append(1e3 * (time.perf_counter() - t0))
    res["numpy_restatement_host"] = {"median_ms": round(statistics.median(host), 1), "min_ms": round(min(host), 1), "max_ms": round(max(host), 1),
                                     "runs": args.host_runs, "cpus": os.cpu_count()}
    res["equals_restatement"] = bool(why is None and ref["voxels"] == m and ref["inside"] == sample["inside"] and
                                     np.array_equal(sample["pc"].cpu().numpy().view(np.uint32), ref["pc"].view(np.uint32)) and
                                     np.array_equal(sample["img"].cpu().numpy(), ref["img"]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
