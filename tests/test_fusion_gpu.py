"""cofi_fuse_cloud_image (cofii2p_amd.fusion) on the MI355X against the float64 restatement tests/fusion_refs.py, on scenes from which the
points whose answer fp32 could legitimately flip have been removed: index, flags, camera and stats EQUAL, depth within 2 ulp of the fp32
rounding of the winner's float64 z, colour within the bound fusion_refs derives from the projection body's operation count; then
reproducibility, graph capture, tie and failure rules, strided operands, and the way up through forward_async and FrameBatcher.

Every call runs into poisoned outputs and a workspace filled with junk.  Error-path tests check refusals made on the host only."""
import numpy as np
import pytest
import torch

import fusion_refs as fr
from test_rig_gpu import CAMERAS, cloud, image, model, rig_inputs  # noqa: F401  (model: the fixture)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
OUT = ("depth", "index", "flags", "color", "camera", "stats")


@pytest.fixture(scope="module")
def fusion():
    from cofii2p_amd import fusion as f

    return f


def upload(sc):
    return {k: torch.from_numpy(np.array(sc[k])).to(DEV) for k in ("points", "images", "pose", "K", "result")}


def poisoned(fusion, S, N, F, H, W, Ci):
    b = fusion.FusionBuffers(S, N, F, H, W, Ci, DEV)
    b.depth.fill_(float("nan"))
    b.index.fill_(123456)
    b.flags.fill_(0xAA)
    b.color.fill_(-7.0)
    b.camera.fill_(77)
    b.stats.fill_(99)
    b.ws.fill_(0x0123456789ABCDE)
    return b


def run(fusion, t, cameras, splat, result="own", buffers=None, **kw):
    """the fusion of uploaded scene tensors into poisoned buffers -> (numpy outputs, buffers)"""
    F, Ci, H, W = t["images"].shape
    S = F // cameras
    N = t["points"].numel() // 3 // S
    b = buffers if buffers is not None else poisoned(fusion, S, N, F, H, W, Ci)
    args = dict(fr.DEFAULTS, **kw)
    fusion.fuse_into(t["points"], t["images"], t["pose"], t["K"], b, result=t["result"] if isinstance(result, str) else result, cameras=cameras,
                     splat=splat, **args)
    torch.cuda.synchronize()
    return {k: getattr(b, k).cpu().numpy() for k in OUT}, b


def assert_equals_reference(got, ref, sc, tag=""):
    for k in ("index", "flags", "camera", "stats"):
        assert np.array_equal(got[k], ref[k]), (tag, k, int((got[k] != ref[k]).sum()))
    hit = ref["index"] >= 0
    want = ref["depth"].astype(np.float32)
    assert (got["depth"][~hit] == 0).all(), tag
    ulps = np.abs(got["depth"][hit].astype(np.float64) - want[hit]) / np.spacing(want[hit])
    worst_ulp = float(ulps.max()) if ulps.size else 0.0
    err, bound = np.abs(got["color"] - ref["color"]), fr.color_bound(sc, ref)
    seen = ref["camera"] >= 0
    ratio = float((err[seen] / bound[seen]).max()) if seen.any() else 0.0
    print("%s depth: worst %.2f ulp; colour: worst error %.3e, worst error / bound %.3f (bound up to %.3e)"
          % (tag, worst_ulp, float(err.max()), ratio, float(bound.max())))
    assert worst_ulp <= 2.0, (tag, worst_ulp)
    assert (got["color"][~seen] == 0).all(), tag
    assert (err <= bound).all(), (tag, float(err.max()), ratio)


def assert_same(a, b, tag=""):
    for k in OUT:
        assert np.array_equal(a[k], b[k], equal_nan=True), (tag, k)


# ------------------------------------------------------------------------------------------------ against the reference
@pytest.mark.parametrize("case", fr.CASES, ids=fr.CASE_IDS)
def test_equals_the_reference(fusion, case):
    sc, ref = fr.scene(case)
    got, _ = run(fusion, upload(sc), sc["cameras"], sc["splat"])
    assert_equals_reference(got, ref, sc, fr.CASE_IDS[fr.CASES.index(case)])


def test_two_runs_and_a_captured_graph_are_bit_equal(fusion):
    sc, ref = fr.scene(fr.CASES[7])
    t = upload(sc)
    a, _ = run(fusion, t, sc["cameras"], sc["splat"])
    b, _ = run(fusion, t, sc["cameras"], sc["splat"])
    assert_same(a, b, "second run")
    S, N = t["points"].shape[:2]
    F, Ci, H, W = t["images"].shape
    buf = poisoned(fusion, S, N, F, H, W, Ci)
    args = dict(result=t["result"], cameras=sc["cameras"], splat=sc["splat"], **fr.DEFAULTS)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fusion.fuse_into(t["points"], t["images"], t["pose"], t["K"], buf, **args)      # warm-up: nothing is allocated inside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        fusion.fuse_into(t["points"], t["images"], t["pose"], t["K"], buf, **args)
    for rep in range(2):
        for k in OUT:
            getattr(buf, k).fill_(5)
        buf.ws.fill_(rep + 1)
        graph.replay()
        torch.cuda.synchronize()
        assert_same(a, {k: getattr(buf, k).cpu().numpy() for k in OUT}, "replay %d" % rep)


def test_duplicates_go_to_the_lower_id(fusion):
    sc, ref0 = fr.scene(fr.CASES[3])                                            # splat 0: one point per pixel
    pts = np.array(sc["points"])
    winners = np.unique(ref0["index"][0][ref0["index"][0] >= 0])
    hi = winners[winners > 128][:6]
    lo = np.array([2, 9, 30, 31, 77, 100])
    lo = lo[~np.isin(lo, winners)][:len(hi)]
    hi = hi[:len(lo)]
    assert len(lo) >= 3
    pts[0, lo] = pts[0, hi]                                                     # exact copies of winning points at lower ids
    dup = dict(sc, points=pts)
    ref = fr.ref_of(dup, 0)
    assert not ref["unstable"].any()                                            # exact duplicates are no near-ties
    got, _ = run(fusion, upload(dup), sc["cameras"], 0)
    assert_equals_reference(got, ref, dup, "duplicates")
    for a, b in zip(lo, hi):
        assert (got["index"][0] == a).sum() == 1 and (got["index"][0] == b).sum() == 0
        assert got["flags"][0, a] == 3 and got["flags"][0, b] == 3


def test_failed_image_and_nan_pose_leave_their_maps_empty(fusion):
    sc, ref = fr.scene(fr.CASES[7])                                             # S = 2, C = 2; image 3 has result 0
    t = upload(sc)
    base, _ = run(fusion, t, 2, sc["splat"])
    assert base["stats"][3].tolist() == [0, 0, 0, 0] and (base["index"][3] == -1).all() and (base["depth"][3] == 0).all()
    assert (base["flags"][3] == 0).all()
    # a NaN pose on image 0, whose result still says success: nothing of it is in picture
    pose = np.array(sc["pose"])
    pose[0, 4] = np.nan
    got, _ = run(fusion, dict(t, pose=torch.from_numpy(pose).to(DEV)), 2, sc["splat"])
    result = np.array(sc["result"][:, 0])
    result[0] = 0
    want = fr.fuse_ref(sc["points"], sc["images"], sc["pose"], sc["K"], result, 2, splat=sc["splat"], **fr.DEFAULTS)
    assert_equals_reference(got, want, sc, "NaN pose")
    assert got["stats"][0].tolist() == [0, 0, 0, 0] and (got["index"][0] == -1).all() and (got["flags"][0] == 0).all()
    for k in ("depth", "index", "flags", "stats"):                              # the other images are untouched
        assert np.array_equal(got[k][1:], base[k][1:]), k
    assert np.array_equal(got["color"][1], base["color"][1]) and np.array_equal(got["camera"][1], base["camera"][1])
    assert set(np.unique(got["camera"][0])) <= {-1, 1}
    # no result tensor at all: every image takes part
    every, _ = run(fusion, t, 2, sc["splat"], result=None)
    assert_equals_reference(every, fr.fuse_ref(sc["points"], sc["images"], sc["pose"], sc["K"], None, 2, splat=sc["splat"], **fr.DEFAULTS), sc, "no result")
    assert every["stats"][3, 0] > 0


@pytest.mark.parametrize("splat", [1, 3])
def test_splat_is_clipped_at_all_four_borders(fusion, splat):
    H, W = 9, 11
    K = np.array([[[4.0, 0, 2.5], [0, 4.0, 2.0], [0, 0, 1]]], dtype=np.float32)      # with k_scale 2: fx = fy = 8, cx = 5, cy = 4
    uv = np.array([[0.2, 0.1], [W - 1.2, 0.2], [0.1, H - 1.2], [W - 0.8, H - 0.9], [-0.3, 4.2], [5.1, H - 0.7]])   # corners and two edges
    z = np.array([2.0, 3.0, 4.0, 5.0, 6.0, 7.0])
    pts = np.stack([z * (uv[:, 0] - 5) / 8, z * (uv[:, 1] - 4) / 8, z], 1).astype(np.float32)[None]
    sc = {"points": pts, "images": fr.smooth_images(1, 3, H, W), "pose": np.concatenate([np.eye(3).reshape(9), np.zeros(3)])[None].astype(np.float32),
          "K": K, "result": np.ones((1, 3), dtype=np.int32), "cameras": 1}
    ref = fr.ref_of(sc, splat)
    assert not ref["unstable"].any() and (ref["flags"][0] == 3).all()
    got, _ = run(fusion, upload(sc), 1, splat)
    assert_equals_reference(got, ref, sc, "splat %d at the borders" % splat)
    n = splat + 1
    for i in range(4):                                                          # a corner point keeps (splat + 1)^2 pixels
        assert (got["index"][0] == i).sum() == n * n, (i, int((got["index"][0] == i).sum()))
    assert got["index"][0][0, 0] == 0 and got["index"][0][0, W - 1] == 1 and got["index"][0][H - 1, 0] == 2 and got["index"][0][H - 1, W - 1] == 3


def test_strided_operands_are_read_in_place(fusion):
    sc, ref = fr.scene(fr.CASES[7])
    t = upload(sc)
    base, _ = run(fusion, t, 2, sc["splat"])
    F = t["pose"].shape[0]
    big = torch.full((F, 20), float("nan"), device=DEV)
    big[:, 4:16] = t["pose"]
    counts = torch.full((F, 5), 0, dtype=torch.int32, device=DEV)               # zeros beside the column that is read
    counts[:, 2] = t["result"][:, 0]
    view, col = big[:, 4:16], counts[:, 2]
    assert not view.is_contiguous() and col.stride(0) == 5
    got, _ = run(fusion, dict(t, pose=view), 2, sc["splat"], result=col)
    assert_same(base, got, "pose inside a larger buffer, result as a strided column")
    # the pair of views a forward handle holds, and a pair of unrelated tensors (joined into a new buffer)
    pair = (view[:, :9].view(F, 3, 3), view[:, 9:])
    got, _ = run(fusion, dict(t, pose=pair), 2, sc["splat"])
    assert_same(base, got, "R / t views")
    got, _ = run(fusion, dict(t, pose={"R": pair[0].clone(), "t": pair[1].clone()}), 2, sc["splat"])
    assert_same(base, got, "R / t copies")
    got, _ = run(fusion, dict(t, points=t["points"].reshape(-1, 3), K=np.array(sc["K"])), 2, sc["splat"])       # flat rows, a host K
    assert_same(base, got, "flat points, host K")


def test_python_refusals_with_device_operands(fusion):
    """host-side refusals only: nothing here reaches a launch"""
    from cofii2p_amd._lib import CofiError

    sc, _ = fr.scene(fr.CASES[3])                                               # S = 2, C = 2, N = 257, 16 x 24, Ci = 3
    t = upload(sc)
    b = fusion.FusionBuffers(2, 257, 4, 16, 24, 3, DEV)
    ok = dict(points=t["points"], images=t["images"], pose=t["pose"], K=t["K"], buffers=b, result=t["result"], cameras=2, splat=1)
    bad = [dict(splat=4), dict(splat=-1), dict(splat=1.0), dict(cameras=3), dict(cameras=0), dict(z_near=0.0), dict(rel_tol=-1.0), dict(abs_tol=float("nan")),
           dict(k_scale=0.0), dict(points=t["points"][:, :256]), dict(points=t["points"].double()), dict(points=t["points"].cpu()),
           dict(images=t["images"][:, :, :, :23]), dict(images=t["images"][:3]), dict(pose=t["pose"][:, :11]), dict(pose=t["pose"].t()),
           dict(pose=t["pose"][:3]), dict(K=t["K"][:3]), dict(K=np.eye(4)), dict(result=t["result"].long()), dict(result=t["result"][:3]),
           dict(buffers=fusion.FusionBuffers(2, 257, 4, 16, 24, 1, DEV)), dict(buffers=fusion.FusionBuffers(1, 514, 4, 16, 24, 3, DEV)),
           dict(buffers=fusion.FusionBuffers(2, 257, 4, 16, 24, 3, "cpu")), dict(buffers=None)]
    before = {k: getattr(b, k).clone() for k in OUT}
    for change in bad:
        with pytest.raises(CofiError):
            fusion.fuse_into(**dict(ok, **change))
    torch.cuda.synchronize()
    assert all(torch.equal(before[k], getattr(b, k)) for k in OUT)              # nothing was written


# ------------------------------------------------------------------------------------------------ through the public interface
def pipeline_K(B):
    """intrinsics of the fine map (half the 160 x 512 model image), as pose_K expects them"""
    return torch.from_numpy(np.stack([np.array([[300.0 + 4 * f, 0, 128.0], [0, 296.0 + 2 * f, 40.0 + f], [0, 0, 1.0]]) for f in range(B)]).astype(np.float32)).to(DEV)


def standalone(fusion, h, points0, img, Ks, cameras):
    """fusion.fuse on the handle's own poses, the submission's points and images"""
    b = fusion.fuse(points0, img, h["pose"], Ks, result=h["pose"]["result"], cameras=cameras, k_scale=2.0)
    torch.cuda.synchronize()
    return b


def assert_buffers_equal(a, b, tag=""):
    for k in OUT:
        assert torch.equal(getattr(a, k), getattr(b, k)), (tag, k)


@pytest.mark.parametrize("mode", ["stack", "rig", "rig_pose"])
def test_forward_async_fuses_behind_the_pose_tail(model, fusion, mode):
    import rig_pose_refs as rr
    from cofii2p_amd._lib import CofiError

    rig_in, rep, img = rig_inputs()
    B, iters = img.shape[0], 500
    Ks = pipeline_K(B)
    pyr, C = (rep, 1) if mode == "stack" else (rig_in, CAMERAS)
    kw = {} if C == 1 else {"cameras": C}
    if mode == "rig_pose":
        kw["rig_extrinsics"] = rr.rig_extrinsics_around(CAMERAS, np.random.default_rng(77))
    S, N = B // C, pyr["points"][0].shape[0] // (B // C)
    slot = {"stack": 21, "rig": 22, "rig_pose": 23}[mode]
    model.enable_graphs(True)
    try:
        buf = poisoned(fusion, S, N, B, img.shape[2], img.shape[3], 3)
        for rep_ in range(2):                                                   # the second submission replays the slot's graph
            h = model.forward_async(slot, pyr, img, pose_K=Ks, pose_iterations=iters, pose_seed=5, fuse_into=buf, **kw)
            model.finish(h)
            assert h["fusion"] is buf and set(h["pose"]) == {"result", "R", "t", "inliers"}
            want = standalone(fusion, h, pyr["points"][0], img, Ks, C)
            assert_buffers_equal(buf, want, "%s, submission %d" % (mode, rep_))
        st = buf.stats.cpu().numpy()
        ok = h["pose"]["result"][:, 0].cpu().numpy() != 0
        print("%s: results %s, stats %s" % (mode, ok.astype(int).tolist(), st.tolist()))
        assert (st[~ok] == 0).all() and (st[:, 3] == 0).all() and (st[:, 1] <= st[:, 0]).all()
        # the same submission without the fusion: every output and pose bit-equal, no "fusion" in the handle
        snap = [[t_.clone() for t_ in o.values() if torch.is_tensor(t_)] for o in h["out"]] + [[h["pose"][k].clone() for k in ("result", "R", "t", "inliers")]]
        h2 = model.forward_async(slot, pyr, img, pose_K=Ks, pose_iterations=iters, pose_seed=5, **kw)
        model.finish(h2)
        assert "fusion" not in h2
        snap2 = [[t_ for t_ in o.values() if torch.is_tensor(t_)] for o in h2["out"]] + [[h2["pose"][k] for k in ("result", "R", "t", "inliers")]]
        assert len(snap) == len(snap2) and all(len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b)) for a, b in zip(snap, snap2))
        # refusals, before anything is enqueued: the slot stays usable
        with pytest.raises(CofiError):
            model.forward_async(slot, pyr, img, fuse_into=buf, **kw)                                                  # no pose_K
        with pytest.raises(CofiError):
            model.forward_async(slot, pyr, img, pose_K=Ks, fuse_into=fusion.FusionBuffers(S, N - 1, B, img.shape[2], img.shape[3], 3, DEV), **kw)
        with pytest.raises(CofiError):
            model.forward_async(slot, pyr, img, pose_K=Ks, fuse_into=fusion.FusionBuffers(S, N, B, img.shape[2], img.shape[3] // 2, 3, DEV), **kw)
        with pytest.raises(CofiError):
            model.forward_async(slot, pyr, img, pose_K=Ks, fuse_into={"depth": buf.depth}, **kw)
    finally:
        model.enable_graphs(False)


@pytest.mark.parametrize("C", [1, 3])
def test_frame_batcher_fusion_result(model, fusion, C):
    import rig_pose_refs as rr
    from cofii2p_amd.serving import FrameBatcher

    B, iters = 2 * C, 500
    Ks = pipeline_K(C).cpu().numpy()
    model.enable_graphs(True)
    try:
        if C == 1:
            fb = FrameBatcher(model, batch=B, streams=1, ring=2, slot_base=90, pose=True, pose_iterations=iters, fuse=True)
            tickets = [fb.submit(cloud(31), image(40), K=Ks[0])]
        else:
            E = rr.rig_extrinsics_around(C, np.random.default_rng(77))
            fb = FrameBatcher(model, batch=B, cameras=C, streams=1, ring=2, slot_base=94, pose=True, pose_iterations=iters, fuse=True, rig_extrinsics=E)
            tickets = fb.submit_rig(cloud(31), torch.cat([image(i) for i in (40, 41, 42)]), K=Ks)
        got = [fb.fusion_result(tk) for tk in tickets]                          # the first call flushes the half-filled stack
        j = tickets[0][0]
        st_, poses = fb._stacks[j], fb._poses[j]
        want = fusion.fuse(st_.pyr["points"][0], st_.img, poses, fb._K[j], result=poses["result"], cameras=C, k_scale=2.0)
        torch.cuda.synchronize()
        N = want.N
        for c, (tk, g) in enumerate(zip(tickets, got)):
            assert set(g) == {"depth", "index", "flags", "stats", "color", "camera"}
            img_of = slice(0, C) if C > 1 else 0
            for k in ("depth", "index", "flags", "stats"):
                assert torch.equal(g[k], getattr(want, k)[img_of]), (c, k)
            assert torch.equal(g["color"], want.color[0]) and torch.equal(g["camera"], want.camera[0])
            assert tuple(g["color"].shape) == (N, 3) and tuple(g["depth"].shape) == ((C, 160, 512) if C > 1 else (160, 512))
        with pytest.raises(RuntimeError):
            FrameBatcher(model, batch=B, cameras=C, pose=True).fusion_result(tickets[0])
        with pytest.raises(ValueError):
            FrameBatcher(model, batch=B, cameras=C, fuse=True)
    finally:
        model.enable_graphs(False)
