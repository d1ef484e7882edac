"""The float64 reference of the cloud / image fusion (tests/fusion_refs.py) held to its own invariants and to a restatement of the reference
project's crop mask, the removal cap of every scene the GPU tests use, and the host-only parts of the fusion surface (workspace query,
header and binding table, refusals made before a device is touched)."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import fusion_refs as fr
from cofii2p_amd import _lib, fusion


# ------------------------------------------------------------------------------------------------ the generator stays inside its cap
@pytest.mark.parametrize("case", fr.CASES, ids=fr.CASE_IDS)
def test_removal_cap_and_scene_content(case):
    sc, ref = fr.scene(case)
    S, N, _ = sc["points"].shape
    print("%s: removed %d of %d points (cap %d)" % (fr.CASE_IDS[fr.CASES.index(case)], sc["removed"], S * N, int(0.02 * S * N)))
    assert sc["removed"] <= 0.02 * S * N
    assert not ref["unstable"].any()                                            # the removal settled
    if N >= 63:                                                                 # the scene shows what it is meant to show
        live = sc["result"][:, 0] != 0
        assert (ref["stats"][live, 0] > 0).all() and (ref["stats"][live, 1] < ref["stats"][live, 0]).all()       # something is hidden
        assert (ref["z"] < 0).any() and np.isnan(sc["points"]).any()
        assert ((ref["flags"] & 1) == 0).any()
    if sc["result"].shape[0] >= 2:
        assert (sc["result"][:, 0] == 0).sum() == 1


# ------------------------------------------------------------------------------------------------ invariants of the reference
@pytest.mark.parametrize("case", fr.CASES, ids=fr.CASE_IDS)
def test_reference_invariants(case):
    sc, ref = fr.scene(case)
    F, H, W = ref["index"].shape
    C = sc["cameras"]
    for f in range(F):
        ids = ref["index"][f][ref["index"][f] >= 0]
        assert (ref["flags"][f, ids] & 1).all()                                 # every id in the map is in picture ...
        if sc["splat"] == 0:
            # ... and visible: with splat 0 a pixel's winner is the minimum of its OWN pixel and passes its own gate.  (With a splat a point
            # can own a neighbouring pixel while a nearer point, splatted from the other side, hides it at its own: include/cofi_hip.h.)
            assert (ref["flags"][f, ids] & 2).all()
            assert len(np.unique(ids)) == len(ids) == ref["stats"][f, 2]        # one point per hit pixel
            assert ref["stats"][f, 2] <= ref["stats"][f, 1]
        assert ((ref["flags"][f] & 2) <= 2 * (ref["flags"][f] & 1)).all()       # visible implies in picture
        assert ((ref["depth"][f] > 0) == (ref["index"][f] >= 0)).all()
    seen = ref["camera"] >= 0
    assert (ref["color"][~seen] == 0).all()
    for s in range(seen.shape[0]):
        for i in np.nonzero(seen[s])[0][:50]:
            assert ref["flags"][s * C + ref["camera"][s, i], i] & 2


def test_wall_hides_the_scatter():
    """a fronto-parallel wall at z = 3 over the whole picture: of the scatter behind it nothing is visible, every wall point is"""
    rng = np.random.default_rng(5)
    H, W, n = 16, 24, 400
    K = np.array([[[10.0, 0, 5.75], [0, 10.0, 3.75], [0, 0, 1]]], dtype=np.float32)
    u, v = rng.uniform(0.1, W - 1.1, 2 * n), rng.uniform(0.1, H - 1.1, 2 * n)
    z = np.concatenate([np.full(n, 3.0), rng.uniform(6.0, 20.0, n)])
    pts = np.stack([z * (u - 11.5) / 20.0, z * (v - 7.5) / 20.0, z], 1).astype(np.float32)[None]
    pose = np.concatenate([np.eye(3).reshape(9), np.zeros(3)])[None].astype(np.float32)
    ref = fr.fuse_ref(pts, fr.smooth_images(1, 1, H, W), pose, K, None, 1, splat=1, **fr.DEFAULTS)
    covered = ref["index"][0] >= 0
    assert covered.mean() > 0.95
    assert (ref["flags"][0, :n] == 3).all()
    hidden = ref["flags"][0, n:]
    rows, cols = np.round(v[n:]).astype(int), np.round(u[n:]).astype(int)
    behind_wall = ref["index"][0][rows, cols] < n                               # the scatter point's own pixel is a wall pixel
    assert behind_wall.mean() > 0.9 and (hidden[behind_wall] == 1).all()        # in picture, not visible
    assert (ref["index"][0][covered] < n).mean() > 0.95


def test_duplicates_resolve_to_the_lower_id():
    sc = fr.raw_scene(3, 200, 16, 24, 1, 1, 1)
    pts = sc["points"].copy()
    ref0 = fr.fuse_ref(pts, sc["images"], sc["pose"], sc["K"], None, 1, splat=0, **fr.DEFAULTS)
    winners = np.unique(ref0["index"][0][ref0["index"][0] >= 0])
    hi = winners[winners > 100][:5]
    assert len(hi) == 5
    lo = np.array([3, 17, 40, 41, 99])                                          # copies of five winning points at lower ids
    pts[0, lo] = pts[0, hi]
    ref = fr.fuse_ref(pts, sc["images"], sc["pose"], sc["K"], None, 1, splat=0, **fr.DEFAULTS)
    for a, b in zip(lo, hi):
        assert (ref["index"][0] == a).sum() == 1 and (ref["index"][0] == b).sum() == 0
        assert ref["flags"][0, a] == 3 and ref["flags"][0, b] == 3              # both pass the gate: they share the minimum


@pytest.mark.parametrize("case", [fr.CASES[3], fr.CASES[5], fr.CASES[8]], ids=[fr.CASE_IDS[i] for i in (3, 5, 8)])
def test_in_picture_rule_is_the_crop_mask(case):
    """on the points in front of the camera the in-picture bit equals crop_pc_with_img's mask (np.round of K X / z, 0 <= px <= W - 1)"""
    sc, ref = fr.scene(case)
    F, H, W = ref["index"].shape
    C = sc["cameras"]
    for f in range(F):
        if sc["result"][f, 0] == 0:
            continue
        P = sc["points"][f // C].astype(np.float64)
        R, t = sc["pose"][f, :9].astype(np.float64).reshape(3, 3), sc["pose"][f, 9:].astype(np.float64)
        cam = P @ R.T + t
        front = cam[:, 2] > fr.DEFAULTS["z_near"]
        fx, fy, cx, cy = ref["k4"][f]
        mask = fr.crop_mask(cam[front], np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]]), H, W)
        assert np.array_equal(mask, (ref["flags"][f, front] & 1).astype(bool))
        assert not (ref["flags"][f, ~front] & 1).any()


def test_color_bound_is_small_and_positive():
    sc, ref = fr.scene(fr.CASES[7])
    b = fr.color_bound(sc, ref)
    seen = ref["camera"] >= 0
    assert (b[seen] > 0).all() and b.max() < 1e-5 and (b[~seen] == 0).all()


# ------------------------------------------------------------------------------------------------ host-only checks
def test_workspace_query():
    lib = _lib.load()
    assert lib.cofi_fuse_workspace(16, 160, 512) == 16 * 160 * 512 * 8
    assert lib.cofi_fuse_workspace(1, 5, 7) == 280
    assert lib.cofi_fuse_workspace(3, 1, 1) == 24
    for bad in ((0, 5, 7), (1, 0, 7), (1, 5, -1), (-2, 5, 7)):
        assert lib.cofi_fuse_workspace(*bad) == 0
    assert lib.cofi_fuse_workspace(1, 46341, 46341) == 0                        # H * W beyond 31 bits
    assert lib.cofi_fuse_workspace(65535, 32768, 2) == 0                        # F * H * W beyond 31 bits
    assert lib.cofi_fuse_workspace(2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1) == 0
    assert lib.cofi_fuse_workspace(1, 2 ** 31 - 1, 1) == 8 * (2 ** 31 - 1)


def test_header_and_binding_table():
    assert set(_lib.header_symbols()) == set(_lib.SIGNATURES)
    assert {"cofi_fuse_cloud_image", "cofi_fuse_workspace"} <= set(_lib.SIGNATURES)
    assert _lib.ABI_VERSION == 3                                                # an additive change
    header = (Path(__file__).resolve().parents[1] / "include" / "cofi_hip.h").read_text()
    assert re.search(r"#define COFI_ABI_VERSION 3\b", header)
    for name in ("cofi_fuse_cloud_image", "cofi_fuse_workspace"):
        m = re.search(r"\b%s\(([^;]*)\);" % name, header)
        assert m, name
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert _lib.SIGNATURES["cofi_fuse_workspace"][0] is ctypes.c_size_t


def test_library_refuses_bad_arguments_on_the_host():
    """every refusal of cofi_fuse_cloud_image is made before anything is enqueued: callable without a GPU (the pointers are never read)"""
    lib = _lib.load()
    p = ctypes.c_void_p(4096)
    ok = dict(points=p, N=10, images=4, cameras=2, img=p, Ci=3, H=5, W=7, pose=p, pose_stride=12, result=None, result_stride=0, K=p, k_scale=1.0,
              z_near=0.5, splat=1, rel=0.02, abs=0.05, ws=p, ws_bytes=4 * 5 * 7 * 8, depth=p, index=p, flags=p, color=p, camera=p, stats=p, stream=None)
    cases = [({"splat": 4}, -1), ({"splat": -1}, -1), ({"cameras": 3}, -1), ({"ws_bytes": 4 * 5 * 7 * 8 - 1}, -2), ({"N": 0}, -1),
             ({"pose_stride": 11}, -1), ({"z_near": 0.0}, -1), ({"z_near": float("nan")}, -1), ({"rel": -0.1}, -1),
             ({"images": 65535 * 2, "H": 32768, "W": 1, "ws_bytes": 2 ** 40}, -1)]   # F * H * W beyond 31 bits
    cases += [({k: None}, -1) for k in ("points", "img", "pose", "K", "ws", "depth", "index", "flags", "color", "camera", "stats")]
    for change, want in cases:
        a = dict(ok, **change)
        assert lib.cofi_fuse_cloud_image(*a.values()) == want, change


def test_python_refusals_touch_no_device():
    E = _lib.CofiError
    b = fusion.FusionBuffers(1, 10, 1, 5, 7, 3, "cpu")                          # plain allocations: no device involved
    assert tuple(b.depth.shape) == (1, 5, 7) and tuple(b.color.shape) == (1, 10, 3) and b.ws.numel() * 8 == 280
    for bad in ((1, 10, 3, 5, 7, 0), (2, 10, 3, 5, 7, 3), (1, 0, 1, 5, 7, 3), (1, 10, 1, 46341, 46341, 3)):
        with pytest.raises(E):
            fusion.FusionBuffers(*bad, "cpu")
    pts, img = torch.zeros((10, 3)), torch.zeros((1, 3, 5, 7))
    pose, K = torch.zeros((1, 12)), np.eye(3, dtype=np.float32)[None]
    with pytest.raises(E):
        fusion.fuse_into(pts, img, pose, K, b)                                  # host tensors: there is no CPU path
    with pytest.raises(E):
        fusion.fuse(pts, img, pose, K)
    with pytest.raises(E):
        fusion.fuse_into(pts, img, pose, K, None)


def test_forward_async_and_batcher_refuse_before_a_device():
    from cofii2p_amd.network import CoFiI2P
    from cofii2p_amd.serving import FrameBatcher

    class Opt:
        img_H, img_W, img_fine_resolution_scale, norm = 160, 512, 32, "gn"

    model = CoFiI2P(Opt())                                                      # on the host: nothing below reaches a kernel
    b = fusion.FusionBuffers(1, 16, 1, 160, 512, 3, "cpu")
    pyr = {k: [torch.zeros((16, 3))] for k in ("points", "neighbors", "subsampling", "upsampling")}
    pyr["feats"] = torch.zeros((16, 4))
    with pytest.raises(_lib.CofiError, match="pose_K"):
        model.forward_async(0, pyr, torch.zeros((1, 3, 160, 512)), fuse_into=b)
    with pytest.raises(_lib.CofiError, match="FusionBuffers"):
        model.forward_async(0, pyr, torch.zeros((1, 3, 160, 512)), pose_K=np.eye(3), fuse_into=fusion.FusionBuffers(1, 15, 1, 160, 512, 3, "cpu"))
    with pytest.raises(ValueError, match="pose=True"):
        FrameBatcher(model, batch=2, fuse=True, pose=False)
    with pytest.raises(RuntimeError):
        FrameBatcher(model, batch=2, pose=True).fusion_result((0, 0, 0))
