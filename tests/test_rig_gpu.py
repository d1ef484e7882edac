"""Rig submissions: S clouds under B = S * C images in one forward (forward_async(..., cameras=C)).

What is exact here and what is not.  The two kernels of the feature are copies and index arithmetic: cofi_repeat_frames and
cofi_match_finish_rig are compared bit for bit, the first with torch.repeat_interleave, the second with the existing cofi_match_finish on
cloud tensors expanded by torch.  cameras=1 is the old call, bit for bit.  A whole rig forward against the replicated-cloud stack the
parent can already run is NOT bit-equal and is not asked to be: the point-side GEMMs see S instead of B frames and may take another
tile / split-K plan, exactly as a stacked forward against single frames - so that comparison makes the assertions of
tests/test_forward_gpu.py::test_stack_mode_batch_equals_single_frames (2e-5 on the four dense outputs, equal coarse points, coarse
pixel picks that differ only at near-ties and agree on more than 0.9 of the matches)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from common import TIE, assert_coarse_mismatches_are_ties  # noqa: E402

DEV = "cuda:0"


class Opt:
    img_H, img_W, img_fine_resolution_scale, norm = 160, 512, 32, "gn"


@pytest.fixture(scope="module")
def model():
    """the exact-fp32 GEMMs, as the model of tests/test_forward_gpu.py whose stack-mode assertions are reused here"""
    from cofii2p_amd import ops
    from cofii2p_amd.network import CoFiI2P

    saved, ops.GEMM_MODE = ops.GEMM_MODE, "f32"
    yield CoFiI2P(Opt()).to(DEV)
    ops.GEMM_MODE = saved


def maxdiff(a, b):
    return float((a.detach().cpu().float() - torch.as_tensor(b).detach().cpu().float()).abs().max())


@functools.lru_cache(maxsize=None)
def cloud(fid):
    """the pyramid of make_frame(fid, 4096), built as test_stack_mode_batch_equals_single_frames builds it"""
    from cofii2p_amd.preprocess import build_pyramid
    from cofii2p_amd.synth import make_frame, subsample_indices

    fr = make_frame(fid, 4096)
    sub = [torch.from_numpy(s).to(DEV) for s in subsample_indices(4096, 5, seed=fid)]
    pyr = build_pyramid(torch.from_numpy(fr.points).to(DEV), sub)
    pyr["feats"] = torch.from_numpy(fr.feats).to(DEV)
    return pyr


@functools.lru_cache(maxsize=None)
def image(fid):
    from cofii2p_amd.synth import make_frame

    return torch.from_numpy(make_frame(fid, 4096).img)[None].to(DEV)


CLOUDS, CAMERAS, IMAGES = (31, 32), 3, (40, 41, 42, 43, 44, 45)


def rig_inputs():
    """S = 2 clouds, C = 3 images each -> (the rig input, the replicated-cloud stack of 6 the parent runs, the images)"""
    from cofii2p_amd.network import CoFiI2P

    imgs = [image(i) for i in IMAGES]
    for a in range(len(imgs)):
        for b in range(a):
            assert not torch.equal(imgs[a], imgs[b])
    rig, img = CoFiI2P.stack_frames([cloud(c) for c in CLOUDS], imgs)
    rep, img_rep = CoFiI2P.stack_frames([cloud(CLOUDS[f // CAMERAS]) for f in range(len(imgs))], imgs)
    assert torch.equal(img, img_rep)
    return rig, rep, img


def clone_outs(outs):
    return [[t.clone() for t in o] for o in outs]


def assert_outs_equal(a, b, tag=""):
    assert len(a) == len(b), tag
    for f, (x, y) in enumerate(zip(a, b)):
        assert len(x) == len(y) == 8
        for i, (u, v) in enumerate(zip(x, y)):
            assert u.shape == v.shape and torch.equal(u, v), (tag, f, i)


# ------------------------------------------------------------------------------------------------ 1. repeat_frames
@pytest.mark.parametrize("frames,times", [(1, 1), (1, 5), (3, 2)])
@pytest.mark.parametrize("case", ["128_into_256", "cols3", "src_slice", "unaligned_base"])
def test_repeat_frames_exact(frames, times, case):
    from cofii2p_amd import ops

    n, SENT = 257, -7.25   # rows per frame: no multiple of 64
    g = torch.Generator(device="cpu").manual_seed(100 * frames + times)
    rnd = lambda *shape: torch.randn(*shape, generator=g).to(DEV)
    if case == "128_into_256":     # the token stream: 16-byte path, the right half of the buffer is not the copy's
        src, wide, c0, cols = rnd(frames * n, 128), 256, 0, 128
    elif case == "cols3":          # three floats per row: nothing is 16-byte aligned
        src, wide, c0, cols = rnd(frames * n, 3), 3, 0, 3
    elif case == "src_slice":      # the source is a column slice itself (ld 200, 16-byte aligned rows, 70 = 17 x 4 + 2 columns)
        src, wide, c0, cols = rnd(frames * n, 200)[:, 64:134], 96, 8, 70
    else:                          # aligned leading dimensions, base pointers off by one float
        src, wide, c0, cols = rnd(frames * n, 132)[:, 1:130], 136, 3, 129
    buf = torch.full((frames * times * n, wide), SENT, dtype=torch.float32, device=DEV)
    dst = buf[:, c0:c0 + cols]
    out = ops.repeat_frames(src, dst, frames, times)
    torch.cuda.synchronize()
    assert out.data_ptr() == dst.data_ptr()
    want = src.reshape(frames, n, cols).repeat_interleave(times, 0).reshape(frames * times * n, cols)
    assert torch.equal(dst, want)
    keep = torch.ones(wide, dtype=torch.bool, device=DEV)
    keep[c0:c0 + cols] = False
    assert bool((buf[:, keep] == SENT).all())   # columns outside the slice: untouched


def test_repeat_frames_refuses_mismatched_shapes():
    from cofii2p_amd import ops
    from cofii2p_amd._lib import CofiError

    src = torch.zeros((6, 8), device=DEV)
    with pytest.raises(CofiError):
        ops.repeat_frames(src, torch.zeros((13, 8), device=DEV), 2, 2)
    with pytest.raises(CofiError):
        ops.repeat_frames(src, torch.zeros((12, 4), device=DEV), 2, 2)
    with pytest.raises(CofiError):
        ops.repeat_frames(src, torch.zeros((24, 8), device=DEV), 4, 4)   # 6 rows are no 4 blocks


# ------------------------------------------------------------------------------------------------ 2. match_finish(cameras=C)
def test_match_finish_rig_equals_match_finish_on_expanded_clouds():
    from cofii2p_amd import ops
    from cofii2p_amd._lib import CofiError

    S, C, N4, N1, cap, CF, H2, W2 = 2, 3, 64, 300, 64, 64, 16, 24   # S != C on purpose: f % S would pass with S == C
    B = S * C
    g = torch.Generator(device="cpu").manual_seed(5)
    pts4 = (torch.randn(S * N4, 3, generator=g) * 10).to(DEV)
    pts1 = (torch.randn(S * N1, 3, generator=g) * 10).to(DEV)
    fpc = torch.randn(S * N1, CF, generator=g).to(DEV)
    fmap = torch.randn(B * H2 * W2, CF, generator=g).to(DEV)
    counts = [17, 0, cap, 1, 33, 50]   # one image without matches, one at capacity
    sel = torch.stack([torch.randperm(N4, generator=g)[:cap].sort().values for _ in range(B)]).to(torch.int32).to(DEV)
    xy = torch.stack([torch.stack([torch.randint(0, W2 // 4, (cap,), generator=g), torch.randint(0, H2 // 4, (cap,), generator=g)])
                      for _ in range(B)]).to(torch.float32).to(DEV)
    cnt = torch.tensor([[n, 0] for n in counts], dtype=torch.int32, device=DEV)
    expand = lambda t, n: t.reshape(S, n, -1).repeat_interleave(C, 0).reshape(B * n, -1).contiguous()
    want = ops.match_finish(expand(pts4, N4), expand(pts1, N1), sel, cnt, fmap, H2, W2, xy, expand(fpc, N1), 4.0, frames=B)
    got = ops.match_finish(pts4, pts1, sel, cnt, fmap, H2, W2, xy, fpc, 4.0, frames=B, cameras=C)
    torch.cuda.synchronize()
    names = ("coarse_pts", "patches", "fine_pc", "fine_xy", "best")
    for name, a, b in zip(names, got, want):
        assert a.shape == b.shape and a.dtype == b.dtype, name
        for f, n in enumerate(counts):
            if name == "fine_xy":   # (B, 2, cap): coordinate-major
                assert torch.equal(a[f][:, :n], b[f][:, :n]), (name, f)
            else:
                assert torch.equal(a[f][:n], b[f][:n]), (name, f)
    # the clouds differ, so an image reading the wrong one would show: image 3 (cloud 1) against cloud 0's points
    assert not torch.equal(pts4[sel[3, 0].item()], pts4[N4 + sel[3, 0].item()])
    assert torch.equal(got[0][3][0], pts4[N4 + sel[3, 0].item()])
    with pytest.raises(CofiError):
        ops.match_finish(pts4, pts1, sel, cnt, fmap, H2, W2, xy, fpc, 4.0, frames=B, cameras=4)


# ------------------------------------------------------------------------------------------------ 3. cameras=1 is the old call
def test_cameras_1_is_the_old_call(model):
    from cofii2p_amd.network import CoFiI2P

    stacked, img = CoFiI2P.stack_frames([cloud(f) for f in (31, 32, 33)], [image(f) for f in (31, 32, 33)])
    model.enable_graphs(False)
    old = clone_outs(model.finish(model.forward_async(5, stacked, img)))
    new = clone_outs(model.finish(model.forward_async(5, stacked, img, cameras=1)))
    assert_outs_equal(old, new, "same slot")
    other = model.finish(model.forward_async(6, stacked, img, cameras=1))   # a capture of its own
    assert_outs_equal(old, other, "fresh capture")


# ------------------------------------------------------------------------------------------------ 4. rig == replicated stack
def eager_rig(model, rig, img, cameras):
    """the rig forward launch by launch (no hipGraph): _run_device as forward_async's capture calls it"""
    from cofii2p_amd import ops

    with torch.no_grad(), ops.arithmetic(model.arithmetic):
        P = model._pack(img.device)
        outs = model._run_device(P, rig["points"], rig["neighbors"], rig["subsampling"], rig["upsampling"], rig["feats"], img, "test", None,
                                 None, order=rig.get("order"), cameras=cameras)
    cnt = outs[0]["count_all"].cpu()
    return [model._slice_result(o, int(cnt[f, 0]), int(cnt[f, 1])) for f, o in enumerate(outs)]


def test_rig_equals_replicated_stack(model):
    rig, rep, img = rig_inputs()
    B = img.shape[0]
    model.enable_graphs(False)
    want = clone_outs(model.finish(model.forward_async(7, rep, img)))          # what the parent computes: every cloud repeated per image
    got = clone_outs(model.finish(model.forward_async(8, rig, img, cameras=CAMERAS)))
    sels = [m["sel"].cpu().numpy() for m in model.last_match_frames]
    assert len(got) == len(want) == B
    for k in range(B):
        for i, (a, b) in enumerate(zip(want[k][:4], got[k][:4])):
            d = maxdiff(a, b)
            print("image %d output %d: max |rig - replicated| = %.3g" % (k, i, d))
            assert d < 2e-5, (k, i, d)
        assert want[k][6].shape == got[k][6].shape
        assert torch.equal(want[k][7], got[k][7])
        same = assert_coarse_mismatches_are_ties(got[k][0], got[k][1], sels[k], got[k][6].cpu().numpy(), want[k][6].cpu().numpy(), tie=TIE)
        print("image %d: %d matches, identical coarse picks %.4f" % (k, got[k][6].shape[1], same))
        assert same > 0.9
    # image f saw cloud f // C: the point descriptors of one cloud's images differ (the cross layers mix the image in) ...
    assert not torch.equal(got[0][1], got[1][1])
    # ... launch by launch and replayed from a fresh capture: the same bits
    eager = eager_rig(model, rig, img, CAMERAS)
    assert_outs_equal(got, eager, "eager")
    model.enable_graphs(True)
    try:
        replay = model.finish(model.forward_async(9, rig, img, cameras=CAMERAS))
        assert_outs_equal(got, replay, "graph")
        replay2 = model.finish(model.forward_async(9, rig, img, cameras=CAMERAS))   # the second call only replays
        assert_outs_equal(got, replay2, "graph, replay only")
    finally:
        model.enable_graphs(False)


# ------------------------------------------------------------------------------------------------ 5. the pose tail on a rig
def test_pose_tail_on_a_rig(model):
    from cofii2p_amd import pose

    rig, _, img = rig_inputs()
    B, iters, seed = img.shape[0], 1000, 11
    Ks = torch.from_numpy(np.stack([np.array([[300.0 + 4 * f, 0, 256.0], [0, 296.0 + 2 * f, 80.0 + f], [0, 0, 1.0]]) for f in range(B)]).astype(np.float32)).to(DEV)
    assert tuple(Ks.shape) == (6, 3, 3)
    h = model.forward_async(10, rig, img, cameras=CAMERAS, pose_K=Ks, pose_iterations=iters, pose_seed=seed)
    model.finish(h)
    o0 = h["out"][0]
    want = pose.solve_pnp_ransac_batch(o0["coarse_pts_all"], o0["fine_xy_all"], Ks, o0["count_all"][:, 0], iterations=iters, seed=seed,
                                       coord_major=True)
    torch.cuda.synchronize()
    p = h["pose"]
    assert p["result"].shape == (B, 3)
    for name, a, b in zip(("result", "R", "t", "inliers"), (p["result"], p["R"], p["t"], p["inliers"]), want):
        assert torch.equal(a, b), name
    assert int(o0["count_all"][:, 0].min()) >= 4   # every image had correspondences to solve from


# ------------------------------------------------------------------------------------------------ 6. FrameBatcher(cameras=3)
def test_frame_batcher_rigs(model):
    from cofii2p_amd.network import CoFiI2P
    from cofii2p_amd.preprocess import FrameStack
    from cofii2p_amd.serving import FrameBatcher

    C, B = 3, 6
    rigs = [(cloud(31), torch.cat([image(i) for i in (40, 41, 42)])), (cloud(32), torch.cat([image(i) for i in (43, 44, 45)])),
            (cloud(33), torch.cat([image(i) for i in (46, 47, 48)]))]
    model.enable_graphs(True)
    try:
        fb = FrameBatcher(model, batch=B, cameras=C, streams=2, ring=2, slot_base=30)
        tickets = [fb.submit_rig(pyr, imgs) for pyr, imgs in rigs]   # stack 0 full; stack 1 half full: flushed by result()
        assert all(len(t) == C for t in tickets)
        assert fb.submissions == 1
        with pytest.raises(ValueError):
            fb.submit(rigs[0][0], rigs[0][1][:1])
        with pytest.raises(ValueError):
            fb.submit_rig(rigs[0][0], rigs[0][1][:2])
        # the same stacks filled by hand, the second one padded with a copy of its last rig
        direct = []
        for slot, members in ((40, (0, 1)), (41, (2, 2))):
            st = FrameStack(rigs[0][0], rigs[0][0]["feats"], rigs[0][1][0], B, cameras=C)
            for s, r in enumerate(members):
                pyr = {k: [CoFiI2P._as_idx32(t) if k != "points" else t for t in rigs[r][0][k]] for k in FrameStack.KEYS}
                st.put_cloud(s, pyr, rigs[r][0]["feats"])
                if s == 0:
                    st.put_image(0, rigs[r][1])                      # the rig's (C,3,H,W) at once
                else:
                    for c in range(C):
                        st.put_image(s * C + c, rigs[r][1][c])       # image by image
            direct.append((st, model.finish(model.forward_async(slot, st.pyr, st.img, cameras=C, inputs_stable=True))))
        for r in (2, 0, 1):
            for c in range(C):
                out = fb.result(tickets[r][c])
                want = direct[r // 2][1][(r % 2) * C + c]
                assert len(out) == 8
                for i, (a, b) in enumerate(zip(out, want)):
                    assert a.shape == b.shape and torch.equal(a, b), (r, c, i)
                assert fb.fine_xy(tickets[r][c]).shape == (2, out[7].shape[0])
        assert fb.submissions == 2
        with pytest.raises(ValueError):
            direct[0][0].put(0, rigs[0][0], rigs[0][0]["feats"], rigs[0][1][0])   # put() fills (cloud, image) pairs
    finally:
        model.enable_graphs(False)


def test_frame_batcher_rigs_with_pose(model):
    """pose=True on a rig batcher: every ticket's pose is the per-frame solver on that image's matches with its own camera matrix and
    the seed of its position in the stack; the padding rig of a flushed stack gets the camera matrices of the rig it copies"""
    from cofii2p_amd import pose
    from cofii2p_amd.serving import FrameBatcher

    C, B, iters = 3, 6, 500
    imgs = torch.cat([image(i) for i in (40, 41, 42)])
    Ks = [np.array([[310.0 + 3 * c, 0, 250.0 + c], [0, 305.0, 82.0], [0, 0, 1.0]]) for c in range(C)]
    model.enable_graphs(True)
    try:
        fb = FrameBatcher(model, batch=B, cameras=C, streams=1, ring=2, slot_base=50, pose=True, pose_iterations=iters)
        with pytest.raises(ValueError):
            fb.submit_rig(cloud(31), imgs)                      # pose=True needs the images' K
        tickets = fb.submit_rig(cloud(31), imgs, K=np.stack(Ks))
        for c, tk in enumerate(tickets):
            out = fb.result(tk)                                 # the first call flushes the half-filled stack
            res, R, t, inl = fb.pose_result(tk)
            fxy = fb.fine_xy(tk)
            want = pose.solve_pnp_ransac(out[7].contiguous(), fxy.t().contiguous(), Ks[c], iterations=iters, seed=tk[2])
            assert torch.equal(res.cpu(), want[0].cpu()) and torch.equal(R, want[1]) and torch.equal(t, want[2]) and torch.equal(inl, want[3]), c
        assert torch.equal(fb._K[tickets[0][0]][C:], fb._K[tickets[0][0]][:C])
        pad = fb._poses[tickets[0][0]]                          # the padding rig: the same images and matrices, seeds C .. 2C - 1
        assert pad["result"].shape[0] == B
    finally:
        model.enable_graphs(False)


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals_leave_the_slot_usable(model):
    from cofii2p_amd._lib import CofiError

    rig, rep, img = rig_inputs()
    slot = 11
    model.enable_graphs(False)
    base = clone_outs(model.finish(model.forward_async(slot, rig, img, cameras=CAMERAS)))

    def still_works(tag):
        assert_outs_equal(base, model.finish(model.forward_async(slot, rig, img, cameras=CAMERAS)), tag)
        model.finish(model.forward_async(slot, rep, img))   # ... and so does an ordinary stack in the same slot

    with pytest.raises(CofiError) as e:
        model.forward_async(slot, rig, img, cameras=4)   # 6 images are no rigs of 4
    assert "6" in str(e.value) and "4" in str(e.value)
    still_works("cameras=4")

    bad = dict(rig)
    bad["feats"] = rig["feats"][:-1]                     # 2 * 4096 - 1 rows: S = 2 does not divide them
    with pytest.raises(CofiError) as e:
        model.forward_async(slot, bad, img, cameras=CAMERAS)
    assert "6" in str(e.value) and "3" in str(e.value) and str(bad["feats"].shape[0]) in str(e.value)
    still_works("odd rows")

    with pytest.raises(CofiError):
        model.forward_async(slot, rig, img, cameras=0)
    still_works("cameras=0")

    K = 8
    kpt = torch.zeros((img.shape[0], 2, K), dtype=torch.int64, device=DEV) + 8
    inl = torch.zeros((img.shape[0], K), dtype=torch.int64, device=DEV)
    with pytest.raises((ValueError, CofiError), match="rig"):
        model.forward_val_async(slot, rig, img, kpt, inl, cameras=CAMERAS)
    still_works("forward_val_async")
    with pytest.raises((ValueError, CofiError), match="rig"):
        model.forward_async(slot, rig, img, mode="val", cameras=CAMERAS)
    still_works("mode='val'")
    with pytest.raises((ValueError, CofiError), match="rig"):
        model(rig, img, None, None, None, "test", cameras=CAMERAS)
    still_works("forward()")
