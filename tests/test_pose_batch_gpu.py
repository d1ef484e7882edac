"""The batched pose solver (cofi_pnp_ransac_batch), the registration errors on the device (cofi_pose_errors) and the pose tail of the
stack-mode pipeline (forward_async(pose_K=...), FrameBatcher(pose=True)).

The yardstick of the batched kernels is the per-frame entry (solve_pnp_ransac / cofi_pnp_ransac): both forms run the same device
functions on the same operands in the same order, so every comparison with it is exact - no tolerance anywhere in that part."""
import ctypes

import numpy as np
import pytest
import torch
from scipy.spatial.transform import Rotation

import pnp_oracle as po
from test_pose_cpu import K as K_ORACLE, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CAP = 512
COUNTS = (500, 300, 37, 4, 3, 0)
SHARES = ((0.5, 0.3), (1.0, 0.5), (0.0, 0.0), (0.2, 0.0), (0.5, 0.2), (0.5, 0.2))   # (pixel noise, outlier share) per frame
SEED = 7
ITERS = 512


@pytest.fixture(scope="module")
def pose_mod():
    from cofii2p_amd import pose
    return pose


def frame_K(f):
    """a different camera per frame; every entry is exactly representable in float32 (the per-frame entry takes C floats)"""
    return np.array([[700.0 + 12.5 * f, 0, 256.0 + f], [0, 690.0 + 8.0 * f, 80.0 - 0.5 * f], [0, 0, 1.0]])


def synth_K(rng, n, noise, outliers, Km):
    """tests/test_pose_cpu.py::synth with the camera as an argument"""
    R = Rotation.from_rotvec(rng.normal(size=3) * 0.4).as_matrix()
    t = rng.normal(size=3) * 2 + np.array([0, 0, 12.0])
    X = rng.uniform(-20, 20, (n, 3))
    X[:, 2] = rng.uniform(-5, 5, n)
    Y = X @ R.T + t
    uv = np.stack([Km[0, 0] * Y[:, 0] / Y[:, 2] + Km[0, 2], Km[1, 1] * Y[:, 1] / Y[:, 2] + Km[1, 2]], 1) + rng.normal(size=(n, 2)) * noise
    out = rng.random(n) < outliers
    uv[out] = rng.uniform(0, 512, (int(out.sum()), 2))
    return X.astype(np.float32), uv.astype(np.float32)


def make_batch(seed=20):
    """B = 6 frames in capacity-sized buffers; rows >= count hold finite junk that nothing may read"""
    rng = np.random.default_rng(seed)
    B = len(COUNTS)
    X = rng.uniform(-50, 50, (B, CAP, 3)).astype(np.float32)
    uv = rng.uniform(0, 512, (B, CAP, 2)).astype(np.float32)
    Ks = np.stack([frame_K(f) for f in range(B)]).astype(np.float32)
    for f, n in enumerate(COUNTS):
        if n:
            X[f, :n], uv[f, :n] = synth_K(rng, n, SHARES[f][0], SHARES[f][1], frame_K(f))
    return (torch.from_numpy(X).to(DEV), torch.from_numpy(uv).to(DEV), torch.from_numpy(Ks).to(DEV),
            torch.tensor(COUNTS, dtype=torch.int32, device=DEV))


def per_frame(pose_mod, X, uv, Kf, n, seed, iters=ITERS):
    """the parent's per-frame entry on the frame's valid rows; n == 0 cannot be passed to it: its documented failure output"""
    if n == 0:
        return (torch.tensor([0, 0, -1], dtype=torch.int32, device=DEV), torch.eye(3, device=DEV), torch.zeros(3, device=DEV),
                torch.zeros(0, dtype=torch.uint8, device=DEV))
    return pose_mod.solve_pnp_ransac(X[:n].contiguous(), uv[:n].contiguous(), Kf, iterations=iters, seed=seed)


def assert_frame_equal(got, f, n, want, tag=""):
    res, R, t, mask = got
    wres, wR, wt, wmask = want
    assert torch.equal(res[f].cpu(), wres.cpu()), (tag, f, res[f].cpu().tolist(), wres.cpu().tolist())
    assert torch.equal(R[f], wR) and torch.equal(t[f], wt), (tag, f, (R[f] - wR).abs().max().item(), (t[f] - wt).abs().max().item())
    assert torch.equal(mask[f, :n], wmask), (tag, f)
    assert int(mask[f, n:].sum()) == 0, (tag, f)


@pytest.mark.parametrize("coord_major", [False, True])
@pytest.mark.parametrize("strided_count", [False, True])
def test_batched_equals_per_frame(pose_mod, coord_major, strided_count):
    X, uv, Ks, cnt = make_batch()
    img = uv.transpose(1, 2).contiguous() if coord_major else uv
    if strided_count:   # the forward's (B, 2) count tensor: the valid number at [f, 0]
        c2 = torch.full((len(COUNTS), 2), -7, dtype=torch.int32, device=DEV)
        c2[:, 0] = cnt
        cnt = c2[:, 0]
        assert cnt.stride(0) == 2
    got = pose_mod.solve_pnp_ransac_batch(X, img, Ks, count=cnt, iterations=ITERS, seed=SEED, coord_major=coord_major)
    assert got[0].shape == (6, 3) and got[1].shape == (6, 3, 3) and got[2].shape == (6, 3) and got[3].shape == (6, CAP)
    assert got[0].dtype == torch.int32 and got[3].dtype == torch.uint8 and all(g.is_cuda for g in got)
    for f, n in enumerate(COUNTS):
        want = per_frame(pose_mod, X[f], uv[f], frame_K(f), n, SEED + f)
        assert_frame_equal(got, f, n, want)
        if n < 4:
            assert got[0][f].cpu().tolist() == [0, 0, -1]
            assert torch.equal(got[1][f], torch.eye(3, device=DEV)) and torch.equal(got[2][f], torch.zeros(3, device=DEV))
    assert got[0][:3, 0].cpu().tolist() == [1, 1, 1]   # the frames with enough good matches are solved


def test_batched_count_none_uses_every_row(pose_mod):
    X, uv, Ks, _ = make_batch(21)
    X, uv, Ks = X[:2, :300].contiguous(), uv[:2, :300].contiguous(), Ks[:2].contiguous()
    got = pose_mod.solve_pnp_ransac_batch(X, uv, Ks, iterations=256, seed=3)
    for f in range(2):
        assert_frame_equal(got, f, 300, per_frame(pose_mod, X[f], uv[f], frame_K(f), 300, 3 + f, iters=256))


def test_batched_against_the_oracle(pose_mod):
    """one noisy frame of a batch against oracle/pnp_oracle.py with the frame's seed: the tolerances of
    tests/test_pose_gpu.py::test_pnp_matches_oracle_and_ground_truth (consensus within 3, pose within 2e-3 m / 2e-2 degrees)"""
    rng = np.random.default_rng(11)
    B, f = 3, 1
    X = np.zeros((B, CAP, 3), np.float32)
    uv = np.zeros((B, CAP, 2), np.float32)
    for b in range(B):
        X[b, :500], uv[b, :500], _, _ = synth(rng, n=500, noise=1.0, outliers=0.5)
    Ks = torch.from_numpy(np.stack([K_ORACLE] * B).astype(np.float32)).to(DEV)
    cnt = torch.full((B,), 500, dtype=torch.int32, device=DEV)
    res, R, t, mask = pose_mod.solve_pnp_ransac_batch(torch.from_numpy(X).to(DEV), torch.from_numpy(uv).to(DEV), Ks, count=cnt,
                                                      iterations=ITERS, seed=5)
    ok, Ro, to, masko, hyp = po.solve_pnp_ransac(X[f, :500], uv[f, :500], K_ORACLE, iterations=ITERS, seed=5 + f)
    assert ok and int(res[f, 0]) == 1
    assert abs(int(res[f, 1]) - int(masko.sum())) <= 3
    Pg, Po = pose_mod.pose_matrix(R[f], t[f]), np.eye(4)
    Po[:3, :3], Po[:3, 3] = Ro, to
    d_t, d_r = pose_mod.get_P_diff(Pg, Po)
    assert d_t < 2e-3 and d_r < 2e-2, (d_t, d_r)


def test_frames_are_independent_and_reproducible(pose_mod):
    X, uv, Ks, cnt = make_batch()
    a = pose_mod.solve_pnp_ransac_batch(X, uv, Ks, count=cnt, iterations=ITERS, seed=SEED)
    b = pose_mod.solve_pnp_ransac_batch(X, uv, Ks, count=cnt, iterations=ITERS, seed=SEED)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    # every frame alone, as a batch of one, with the seed its position gave it
    for f in range(len(COUNTS)):
        one = pose_mod.solve_pnp_ransac_batch(X[f:f + 1], uv[f:f + 1], Ks[f:f + 1], count=cnt[f:f + 1], iterations=ITERS, seed=SEED + f)
        for u, v in zip(a, one):
            assert torch.equal(u[f], v[0]), f
    # permuted: position p holds frame perm[p] and draws with seed + p; its result is that of the frame alone with that seed
    perm = [4, 2, 0, 5, 1, 3]
    pt = torch.tensor(perm, device=DEV)
    p = pose_mod.solve_pnp_ransac_batch(X[pt].contiguous(), uv[pt].contiguous(), Ks[pt].contiguous(), count=cnt[pt].contiguous(),
                                        iterations=ITERS, seed=SEED)
    for pos, f in enumerate(perm):
        one = pose_mod.solve_pnp_ransac_batch(X[f:f + 1], uv[f:f + 1], Ks[f:f + 1], count=cnt[f:f + 1], iterations=ITERS, seed=SEED + pos)
        for u, v in zip(p, one):
            assert torch.equal(u[pos], v[0]), (pos, f)


def test_batched_call_is_capturable(pose_mod):
    """no host synchronisation inside the call: it is captured in a hipGraph (a linear chain), the inputs are overwritten in place with
    other frames, one replay gives what the eager call gives on the new inputs"""
    X, uv, Ks, cnt = make_batch(30)
    X2, uv2, Ks2, cnt2 = make_batch(31)
    cnt2 = torch.tensor([450, 250, 30, 4, 2, 1], dtype=torch.int32, device=DEV)   # other counts too
    fxy = uv.transpose(1, 2).contiguous()
    fxy2 = uv2.transpose(1, 2).contiguous()
    args = dict(iterations=ITERS, seed=SEED, coord_major=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # warm-up outside the capture: code objects are loaded
        pose_mod.solve_pnp_ransac_batch(X, fxy, Ks, count=cnt, **args)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = pose_mod.solve_pnp_ransac_batch(X, fxy, Ks, count=cnt, **args)
    X.copy_(X2), fxy.copy_(fxy2), Ks.copy_(Ks2), cnt.copy_(cnt2)
    g.replay()
    torch.cuda.synchronize()
    got = [o.clone() for o in out]
    want = pose_mod.solve_pnp_ransac_batch(X2, fxy2, Ks2, count=cnt2, **args)
    for u, v in zip(got, want):
        assert torch.equal(u, v)
    assert int(want[0][:, 0].sum()) >= 2   # the replay solved real frames


@pytest.fixture(scope="module")
def model():
    from cofii2p_amd.network import CoFiI2P
    import bench

    return CoFiI2P(bench.Opt()).to(DEV)


def test_pose_through_forward_async(pose_mod, model):
    from cofii2p_amd.network import CoFiI2P
    import bench

    B, iters, pose_seed = 4, 1000, 11
    frames = bench.make_inputs(torch.device(DEV), list(range(B)), 20480)
    stacked, imgs = CoFiI2P.stack_frames([fr[0] for fr in frames], [fr[1] for fr in frames])
    Ks = np.stack([np.array([[300.0 + 4 * f, 0, 256.0], [0, 296.0 + 2 * f, 80.0 + f], [0, 0, 1.0]]) for f in range(B)])
    model.enable_graphs(True)
    try:
        plain = [[t.clone() for t in out] for out in model.finish(model.forward_async(60, stacked, imgs))]
        h = model.forward_async(61, stacked, imgs, pose_K=torch.from_numpy(Ks.astype(np.float32)).to(DEV), pose_iterations=iters,
                                pose_seed=pose_seed)
        outs = model.finish(h)
        p = h["pose"]
        assert set(p) == {"result", "R", "t", "inliers"}
        for f in range(B):
            for a, b in zip(outs[f], plain[f]):
                assert torch.equal(a, b), f                      # nothing existing moved
            n = outs[f][7].shape[0]
            want = pose_mod.solve_pnp_ransac(outs[f][7].contiguous(), h["fine_xy"][f].t().contiguous(), Ks[f], iterations=iters,
                                             seed=pose_seed + f)
            assert_frame_equal((p["result"], p["R"], p["t"], p["inliers"]), f, n, want, "forward_async")
        # one (3,3) matrix from the host serves every frame
        h2 = model.forward_async(61, stacked, imgs, pose_K=Ks[0], pose_iterations=iters, pose_seed=pose_seed)
        outs2 = model.finish(h2)
        for f in range(B):
            want = pose_mod.solve_pnp_ransac(outs2[f][7].contiguous(), h2["fine_xy"][f].t().contiguous(), Ks[0], iterations=iters,
                                             seed=pose_seed + f)
            assert_frame_equal(tuple(h2["pose"][k] for k in ("result", "R", "t", "inliers")), f, outs2[f][7].shape[0], want, "broadcast K")
        from cofii2p_amd._lib import CofiError
        with pytest.raises(CofiError):
            model.forward_async(61, stacked, imgs, pose_K=np.eye(4))
    finally:
        model.enable_graphs(False)


def test_frame_batcher_pose(pose_mod, model):
    from cofii2p_amd.serving import FrameBatcher
    import bench

    iters = 800
    frames = bench.make_inputs(torch.device(DEV), list(range(10, 16)), 20480)
    Ks = [np.array([[310.0 + 3 * i, 0, 250.0 + i], [0, 305.0, 82.0], [0, 0, 1.0]]) for i in range(6)]
    model.enable_graphs(True)
    try:
        fb = FrameBatcher(model, batch=4, streams=2, ring=2, slot_base=70, pose=True, pose_iterations=iters)
        tickets = [fb.submit(fr[0], fr[1], K=Ks[i]) for i, fr in enumerate(frames)]   # one full stack, one padded by result()
        for i in (5, 0, 3, 4, 1, 2):
            out = fb.result(tickets[i])
            res, R, t, inl = fb.pose_result(tickets[i])
            n = out[7].shape[0]
            fxy = fb.fine_xy(tickets[i])                        # (2, n): the frame's fine matches, as finish() hands them out
            assert fxy.shape == (2, n)
            f = tickets[i][2]                                   # position in its stack = offset of its seed
            want = pose_mod.solve_pnp_ransac(out[7].contiguous(), fxy.t().contiguous(), Ks[i], iterations=iters, seed=f)
            assert res.shape == (3,) and R.shape == (3, 3) and t.shape == (3,) and inl.shape == (n,)
            assert torch.equal(res.cpu(), want[0].cpu()) and torch.equal(R, want[1]) and torch.equal(t, want[2]) and torch.equal(inl, want[3]), i
        with pytest.raises(ValueError):
            fb.submit(frames[0][0], frames[0][1])               # pose=True needs the frame's K
        # without pose: as before
        fb0 = FrameBatcher(model, batch=4, streams=2, ring=2, slot_base=80)
        t0 = [fb0.submit(fr[0], fr[1]) for fr in frames[:4]]
        ref = [fb.result(tk) for tk in tickets[:4]]
        for tk, r in zip(t0, ref):
            for a, b in zip(fb0.result(tk), r):
                assert torch.equal(a, b)
        with pytest.raises(RuntimeError):
            fb0.pose_result(t0[0])
    finally:
        model.enable_graphs(False)


def test_pose_errors_equal_get_P_diff(pose_mod):
    """both sides compute in fp64 from identical inputs: libm rounding only.  |dRTE| <= 1e-9 m, |dRRE| <= 1e-7 degrees."""
    rng = np.random.default_rng(0)
    n = 256
    pred = np.zeros((n, 12), np.float32)
    gt = np.zeros((n + 1, 4, 4))
    for i in range(n):
        Rp = Rotation.random(random_state=int(rng.integers(1 << 31))).as_matrix()
        pred[i, :9], pred[i, 9:] = Rp.reshape(9), rng.normal(size=3) * 3
        D = np.eye(4)   # the relative pose: middle angle of 'xzy' within +-75 degrees (the sum of |angles| jumps at gimbal lock)
        D[:3, :3] = Rotation.from_euler("xzy", [rng.uniform(-180, 180), rng.uniform(-75, 75), rng.uniform(-180, 180)], degrees=True).as_matrix()
        D[:3, 3] = rng.normal(size=3) * (10.0 ** rng.uniform(-3, 1))
        Pp = np.eye(4)
        Pp[:3, :3], Pp[:3, 3] = pred[i, :9].reshape(3, 3).astype(np.float64), pred[i, 9:].astype(np.float64)
        gt[i] = Pp @ D
    # the gimbal case of tests/test_pose_cpu.py: identity prediction, middle angle 90 degrees
    pred = np.concatenate([pred, np.array([[1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]], np.float32)])
    gt[n] = np.eye(4)
    gt[n, :3, :3] = Rotation.from_euler("xzy", [20, 90, 0], degrees=True).as_matrix()
    want = np.zeros((n + 1, 2))
    for i in range(n + 1):
        Pp = np.eye(4)
        Pp[:3, :3], Pp[:3, 3] = pred[i, :9].reshape(3, 3).astype(np.float64), pred[i, 9:].astype(np.float64)
        want[i] = pose_mod.get_P_diff(Pp, gt[i])
        if i < n:
            assert abs(pose_mod.euler_xzy_deg((np.linalg.inv(Pp) @ gt[i])[:3, :3])[1]) < 80.0
    pg = torch.from_numpy(pred).to(DEV)
    got = pose_mod.pose_errors(pg, torch.from_numpy(gt).to(DEV))
    assert got.shape == (n + 1, 2) and got.dtype == torch.float64 and got.is_cuda
    got = got.cpu().numpy()
    d_rte, d_rre = np.abs(got[:, 0] - want[:, 0]), np.abs(got[:, 1] - want[:, 1])
    print("pose_errors vs get_P_diff: max |dRTE| %.3e m, max |dRRE| %.3e deg (gimbal case %.3e)" % (d_rte.max(), d_rre[:n].max(), d_rre[n]))
    assert d_rte.max() <= 1e-9 and d_rre.max() <= 1e-7, (d_rte.max(), d_rre.max())
    # the (R, t) form and a host P_gt give the same; a float32 P_gt is read as float32
    got2 = pose_mod.pose_errors((pg[:, :9].reshape(-1, 3, 3), pg[:, 9:]), gt).cpu().numpy()
    assert np.array_equal(got, got2)
    gt32 = gt.astype(np.float32)
    got32 = pose_mod.pose_errors(pg, torch.from_numpy(gt32).to(DEV)).cpu().numpy()
    for i in range(0, n, 17):
        Pp = np.eye(4)
        Pp[:3, :3], Pp[:3, 3] = pred[i, :9].reshape(3, 3).astype(np.float64), pred[i, 9:].astype(np.float64)
        w = pose_mod.get_P_diff(Pp, gt32[i].astype(np.float64))
        assert abs(got32[i, 0] - w[0]) <= 1e-9 and abs(got32[i, 1] - w[1]) <= 1e-7


def test_argument_checks(pose_mod):
    from cofii2p_amd import _lib, ops

    E = _lib.CofiError
    X, uv, Ks, cnt = make_batch()
    ok = dict(iterations=64)
    with pytest.raises(E):
        pose_mod.solve_pnp_ransac_batch(X.double(), uv, Ks, **ok)                       # dtype
    with pytest.raises(E):
        pose_mod.solve_pnp_ransac_batch(X, uv.transpose(1, 2).contiguous(), Ks, **ok)    # coordinate-major data without coord_major
    with pytest.raises(E):
        pose_mod.solve_pnp_ransac_batch(X, uv, Ks, coord_major=True, **ok)
    with pytest.raises(E):
        pose_mod.solve_pnp_ransac_batch(X, uv.transpose(1, 2), Ks, coord_major=False, **ok)   # right shape, not contiguous
    with pytest.raises(E):
        pose_mod.solve_pnp_ransac_batch(X, uv, Ks[0], **ok)                             # K (3,3) for six frames
    with pytest.raises(E):
        pose_mod.solve_pnp_ransac_batch(X, uv, Ks[:, :2], **ok)
    with pytest.raises(E):
        pose_mod.solve_pnp_ransac_batch(X, uv, Ks.double(), **ok)                       # a device K is read in place: float32 only
    with pytest.raises(E):
        pose_mod.solve_pnp_ransac_batch(X, uv, Ks, count=cnt.long(), **ok)
    with pytest.raises(E):
        pose_mod.solve_pnp_ransac_batch(X, uv, Ks, count=cnt[:5], **ok)
    with pytest.raises(E):
        pose_mod.solve_pnp_ransac_batch(X.cpu(), uv, Ks, **ok)
    with pytest.raises(E):
        pose_mod.pose_errors(torch.zeros(4, 11, device=DEV), torch.zeros(4, 4, 4, dtype=torch.float64, device=DEV))
    with pytest.raises(E):
        pose_mod.pose_errors(torch.zeros(4, 12, device=DEV), torch.zeros(3, 4, 4, dtype=torch.float64, device=DEV))
    with pytest.raises(E):
        pose_mod.pose_errors(torch.zeros(4, 12, device=DEV), torch.zeros(4, 4, 4, dtype=torch.float16, device=DEV))
    # a host K is uploaded and gives what the device K gives
    a = pose_mod.solve_pnp_ransac_batch(X, uv, Ks, count=cnt, iterations=64, seed=1)
    b = pose_mod.solve_pnp_ransac_batch(X, uv, Ks.cpu().numpy().astype(np.float64), count=cnt, iterations=64, seed=1)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    # the C entry: workspace too small / missing / misaligned -> COFI_EWORKSPACE (-2); bad sizes -> COFI_EINVAL (-1); nothing is launched
    lib = _lib.load()
    B, iters = X.shape[0], 64
    need = lib.cofi_pnp_ransac_batch_workspace(iters, B)
    assert need == 64 + B * iters * 12 * 4 and lib.cofi_pnp_ransac_batch_workspace(0, B) == 0
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    pose = torch.empty((B, 12), device=DEV)
    res = torch.empty((B, 3), dtype=torch.int32, device=DEV)
    mask = torch.empty((B, CAP), dtype=torch.uint8, device=DEV)

    def call(ws_ptr, ws_bytes, n_max=CAP, frames=B, iterations=iters):
        return lib.cofi_pnp_ransac_batch(ops._p(X), 3 * CAP, ops._p(uv), 2 * CAP, 0, ops._p(cnt), 1, ops._p(Ks), n_max, frames, iterations, 8.0, 0, 20,
                                         ws_ptr, ws_bytes, ops._p(pose), ops._p(res), ops._p(mask), ops._stream())

    assert call(ops._p(ws), need - 1) == -2
    assert call(None, need) == -2
    assert call(ctypes.c_void_p(ws.data_ptr() + 4), need) == -2
    assert call(ops._p(ws), need, n_max=0) == -1 and call(ops._p(ws), need, frames=0) == -1 and call(ops._p(ws), need, iterations=0) == -1
    assert call(ops._p(ws), need, n_max=CAP + 1) == -1          # the frame stride is shorter than a frame
    assert call(ops._p(ws), need) == 0
    assert lib.cofi_pose_errors(None, None, 1, 4, None, ops._stream()) == -1
    torch.cuda.synchronize()
