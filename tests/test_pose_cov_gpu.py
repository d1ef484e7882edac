"""Pose uncertainty on the device (cofi_pose_covariance, _batch, _rig, cofi_pose_nees) against the float64 restatement
tests/pose_cov_refs.py, and its way up through forward_async(pose_cov=...) and FrameBatcher(covariance=True).

Every comparison feeds the reference the device's own float32 pose, result and mask: nothing here depends on RANSAC agreeing with
anything.  Tolerances are derived (pose_cov_refs.bound_sums / bound_matrix), with u = 2^-52:
  H, cost      (2 n + 64) u sum_k |J_ki| |J_kj|: two orders of a sum of 2 n terms; a row's terms are the same bits on both sides
  cov, info    16 kappa (2 n + 64) u sqrt(M_ii M_jj), kappa = cond(D^-1/2 H D^-1/2) of the reference (at most 1e6 in every scene here)
  min_pivot    16 kappa (2 n + 64) u: a pivot of the unit-diagonal matrix
The largest error-to-bound ratios seen are printed (-s) and quoted in DESIGN.md."""
import numpy as np
import pytest
import torch

import pose_cov_refs as pc
import rig_pose_refs as rr

pytestmark = pytest.mark.gpu

from test_rig_gpu import CAMERAS, cloud, image, model, rig_inputs  # noqa: E402,F401  (model: the fixture)

DEV = "cuda:0"
ITERS = 256
RATIOS = {}


@pytest.fixture(scope="module")
def pose_mod():
    from cofii2p_amd import pose
    return pose


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def pose12_of(R, t):
    return np.concatenate([host(R).reshape(-1, 9), host(t).reshape(-1, 3)], 1).astype(np.float64)


def note(tag, err, bound):
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = float(np.nanmax(np.where(bound > 0, err / bound, 0.0))) if np.size(err) else 0.0
    RATIOS[tag] = max(RATIOS.get(tag, 0.0), ratio)
    return ratio


def assert_zero(cov, info, stat, tag):
    assert stat[0] == 0 and stat[3] == 0 and not cov.any() and not info.any() and np.isfinite(stat).all(), (tag, stat)


def check(got, ref, sigma_px, tag):
    """one body's (cov, info, stat) as numpy against the reference dict"""
    cov, info, stat = got
    assert np.isfinite(cov).all() and np.isfinite(info).all() and np.isfinite(stat).all(), tag
    assert np.array_equal(cov, cov.T) and np.array_equal(info, info.T), tag
    assert stat[0] == ref["stat"][0] and stat[1] == ref["stat"][1], (tag, stat, ref["stat"])
    n = ref["n"]
    rel = (2 * n + 64) * pc.U
    assert abs(stat[2] - ref["stat"][2]) <= rel * ref["stat"][2], (tag, stat[2], ref["stat"][2])          # cost / (2 n - 6)
    note("cost", np.array(abs(stat[2] - ref["stat"][2])), np.array(rel * ref["stat"][2]))
    if ref["stat"][0] == 0:
        assert_zero(cov, info, stat, tag)
        return
    assert ref["kappa"] <= 1e6, (tag, ref["kappa"])
    assert 0 < stat[3] <= 1 and abs(stat[3] - ref["stat"][3]) <= 16 * ref["kappa"] * rel, (tag, stat[3], ref["stat"][3])
    for name, a, b in (("cov", cov, ref["cov"]), ("info", info, ref["info"])):
        bound = pc.bound_matrix(ref, b)
        r = note(name, np.abs(a - b), bound)
        assert (np.abs(a - b) <= bound).all(), (tag, name, r)
    if sigma_px == 1.0:      # info IS H: the bound of the sums alone
        r = note("H", np.abs(info - ref["H"]), pc.bound_sums(ref))
        assert (np.abs(info - ref["H"]) <= pc.bound_sums(ref)).all(), (tag, "H", r)


def teardown_module(module):
    print("\nlargest error / bound: " + ", ".join("%s %.3g" % kv for kv in sorted(RATIOS.items())))


# ------------------------------------------------------------------------------------------------ 1. frame form
@pytest.mark.parametrize("n,outliers", [(4, 0.3), (4, 0.0), (5, 0.3), (63, 0.3), (64, 0.3), (65, 0.3), (257, 0.3)])
def test_frame_form(pose_mod, n, outliers):
    """n valid rows in a capacity of 300 given by a device count, int(0.3 n) gross outliers (n = 4 with an outlier has no consensus of
    four: the failure path; n = 4 without one: 2 n - 6 = 2)"""
    cap = 300
    X, uv, _ = pc.frame_scene(100 + n, n, cap, outliers)
    Xd, uvd, count = dev(X), dev(uv), torch.tensor([n], dtype=torch.int32, device=DEV)
    K = pc.K_of(pc.FRAME_K4)
    res, R, t, mask = pose_mod.solve_pnp_ransac(Xd, uvd, K, iterations=ITERS, seed=3, count=count)
    solved = int(res[0])
    assert solved == (0 if (n == 4 and outliers) else 1), res.tolist()
    m = host(mask)
    assert not m[n:].any() and (not solved or (m[:n] == 0).any() == (outliers > 0))          # the mask has holes
    cam = pc.frame_cam(X.astype(np.float64), uv.astype(np.float64), pc.FRAME_K4, m)
    cam["X"], cam["uv"], cam["mask"] = cam["X"][:n], cam["uv"][:n], m[:n]
    for sigma_px in (None, 1.0, 2.5):
        got = [pose_mod.pose_covariance(Xd, uvd, K, (R, t), res, mask, sigma_px=sigma_px, count=count) for _ in range(2)]
        for a, b in zip(*got):
            assert torch.equal(a, b)                                                         # bit-reproducible
        assert tuple(got[0][0].shape) == (6, 6) and tuple(got[0][2].shape) == (4,) and got[0][0].dtype == torch.float64
        ref = pc.covariance(pose12_of(R, t)[0], host(res), [cam], sigma_px)
        check([host(g) for g in got[0]], ref, sigma_px, "n=%d sigma=%s" % (n, sigma_px))
        assert ref["stat"][0] == solved


# ------------------------------------------------------------------------------------------------ 2. batch form
B_COUNTS = (0, 3, 4, 37, 70, 70)
B_CAP = 70


def batch_K4(f):
    return (700.0 + 12.5 * f, 690.0 + 8.0 * f, 256.0 + f, 80.0 - 0.5 * f)


def make_batch():
    X, uv = np.zeros((6, B_CAP, 3), np.float32), np.zeros((6, B_CAP, 2), np.float32)
    for f, n in enumerate(B_COUNTS):
        X[f], uv[f], _ = pc.frame_scene(200 + f, n, B_CAP, 0.3 if n > 4 else 0.0, K4=batch_K4(f))
    Ks = np.stack([pc.K_of(batch_K4(f)) for f in range(6)]).astype(np.float32)
    Ks[4, 0, 0] = 0.0                                                                        # one frame with unusable intrinsics
    return X, uv, Ks


@pytest.mark.parametrize("coord_major", [False, True])
def test_batch_form(pose_mod, coord_major):
    X, uv, Ks = make_batch()
    Xd, uvd, Kd = dev(X), dev(uv), dev(Ks)
    img = uvd.transpose(1, 2).contiguous() if coord_major else uvd
    count_all = torch.stack([torch.tensor(B_COUNTS, dtype=torch.int32), torch.full((6,), 999, dtype=torch.int32)], 1).to(DEV)
    count = count_all[:, 0]                                                                  # a strided view, read in place
    assert count.stride(0) == 2
    res, R, t, mask = pose_mod.solve_pnp_ransac_batch(Xd, img, Kd, count, iterations=ITERS, seed=5, coord_major=coord_major)
    assert host(res)[:, 0].tolist() == [0, 0, 1, 1, 0, 1]
    for sigma_px in (None, 1.0):
        cov, info, stat = pose_mod.pose_covariance_batch(Xd, img, Kd, (R, t), res, mask, sigma_px=sigma_px, count=count, coord_major=coord_major)
        again = pose_mod.pose_covariance_batch(Xd, img, Kd, (R, t), res, mask, sigma_px=sigma_px, count=count, coord_major=coord_major)
        assert torch.equal(cov, again[0]) and torch.equal(info, again[1]) and torch.equal(stat, again[2])
        assert tuple(cov.shape) == (6, 6, 6) and tuple(info.shape) == (6, 6, 6) and tuple(stat.shape) == (6, 4)
        p12, m = pose12_of(R, t), host(mask)
        for f, n in enumerate(B_COUNTS):
            tag = "frame %d sigma=%s major=%s" % (f, sigma_px, coord_major)
            got = (host(cov[f]), host(info[f]), host(stat[f]))
            K4 = (float(Ks[f, 0, 0]), float(Ks[f, 1, 1]), float(Ks[f, 0, 2]), float(Ks[f, 1, 2]))
            cam = pc.frame_cam(X[f, :n].astype(np.float64), uv[f, :n].astype(np.float64), K4, m[f, :n])
            check(got, pc.covariance(p12[f], host(res[f]), [cam], sigma_px), sigma_px, tag)
            if int(res[f, 0]) == 0:
                assert_zero(*got, tag)
            if f == 4:
                continue                                                                     # the per-frame entry refuses fx = 0 outright
            # the per-frame call on the frame's slice: capacity-sized with its count, and (n >= 1) the valid rows alone
            one = pose_mod.pose_covariance(Xd[f], uvd[f], Ks[f], (R[f], t[f]), res[f], mask[f], sigma_px=sigma_px, count=count_all[f, :1])
            assert all(torch.equal(a, b) for a, b in zip(one, (cov[f], info[f], stat[f]))), tag
            if n:
                cut = pose_mod.pose_covariance(Xd[f, :n].contiguous(), uvd[f, :n].contiguous(), Ks[f], (R[f], t[f]), res[f],
                                               mask[f, :n].contiguous(), sigma_px=sigma_px)
                assert all(torch.equal(a, b) for a, b in zip(cut, (cov[f], info[f], stat[f]))), tag


# ------------------------------------------------------------------------------------------------ 3. hand-made poses and masks
def test_hand_made_poses_and_masks(pose_mod):
    """through the batch entry point: the failure cases of tests/test_pose_cov_refs_cpu.py, a row behind the camera, a NaN pose, and
    sigma_px given against estimated"""
    X0, uv0, truth = pc.calibration_scene()[1]
    n, F = len(X0), 8
    X, uv = np.repeat(X0[None], F, 0).astype(np.float32), np.repeat(uv0[None], F, 0).astype(np.float32)
    p12 = np.repeat(pc.pose12_f32(*truth)[None], F, 0)
    res = np.tile(np.array([1, n, 0], np.int32), (F, 1))
    mask = np.ones((F, n), np.uint8)
    counts = np.full(F, n, np.int32)
    res[1] = (0, 0, -1)                      # 1: the solver failed
    mask[2, 3:] = 0                          # 2: n = 3
    X[3, :4], uv[3, :4], counts[3] = X[3, :1], uv[3, :1], 4          # 3: four copies of one point
    mask[4] = 0                              # 4: a mask that selects nothing
    X[5, 7] = -X[5, 7]                       # 5: a row behind the camera inside the mask
    p12[6, 4] = np.nan                       # 6: a NaN in the pose
    mask[7, ::3] = 0                         # 7: holes; frame 0: everything
    Ks = np.repeat(pc.K_of(pc.CAL_K4)[None], F, 0).astype(np.float32)
    args = (dev(X), dev(uv), dev(Ks), dev(p12), dev(res, torch.int32), dev(mask, torch.uint8))
    count = dev(counts, torch.int32)
    out = {}
    for sigma_px in (None, 1.0, 2.0):
        got = [host(g) for g in pose_mod.pose_covariance_batch(*args, sigma_px=sigma_px, count=count)]
        assert all(np.isfinite(g).all() for g in got), sigma_px                             # nowhere a NaN or Inf
        out[sigma_px] = got
        for f in range(F):
            k = int(counts[f])
            cam = pc.frame_cam(X[f, :k].astype(np.float64), uv[f, :k].astype(np.float64), pc.CAL_K4, mask[f, :k])
            with np.errstate(all="ignore"):
                ref = pc.covariance(p12[f], res[f], [cam], sigma_px)
            check((got[0][f], got[1][f], got[2][f]), ref, sigma_px, "hand %d sigma=%s" % (f, sigma_px))
        ok, used = got[2][:, 0].tolist(), got[2][:, 1].tolist()
        assert ok == [1, 0, 0 if sigma_px is None else 1, 0, 0, 1, 0, 1], (sigma_px, ok)
        # frame 6: the NaN sits in the second row of R, so every depth is finite, every row is used, and the sums are NaN: ok = 0
        assert used == [n, 0, 3, 4, 0, n - 1, n, n - len(range(0, n, 3))], (sigma_px, used)
    est = out[None]
    for sigma_px in (1.0, 2.0):
        giv = out[sigma_px]
        assert np.array_equal(giv[2][:, 2], est[2][:, 2])                                    # sigma_hat^2 is reported in both
        for f in (0, 5, 7):
            s_hat2 = est[2][f, 2]
            assert 0.7 < s_hat2 < 1.4
            want = est[0][f] * (sigma_px ** 2 / s_hat2)
            dg = np.sqrt(np.diag(want))
            assert (np.abs(giv[0][f] - want) <= 8 * pc.U * dg[:, None] * dg[None, :]).all(), (sigma_px, f)


# ------------------------------------------------------------------------------------------------ 4. rig form
R_CAP = 70


def rig_runs(per_rig):
    """S = 2, C = 3: rig 0 has a camera without rows, rig 1 one with unusable intrinsics; one generator seed gives both rigs the same
    extrinsics (shared), two seeds give each its own (per rig)"""
    a = rr.as_f32(rr.rig_scene(51, (40, 0, 30)))
    b = rr.as_f32(rr.rig_scene(52 if per_rig else 51, (30, 25, 50)))
    assert per_rig or np.array_equal(a["E"], b["E"])
    b["K4s"] = [b["K4s"][0], (0.0,) + b["K4s"][1][1:], b["K4s"][2]]
    return a, b


def pack_rigs(scs, C):
    X, uv = np.zeros((len(scs) * C, R_CAP, 3), np.float32), np.zeros((len(scs) * C, R_CAP, 2), np.float32)
    Ks, counts = np.zeros((len(scs) * C, 3, 3), np.float32), np.zeros(len(scs) * C, np.int32)
    for s, sc in enumerate(scs):
        for c in range(C):
            f, k = s * C + c, len(sc["Xs"][c])
            X[f, :k], uv[f, :k], counts[f], Ks[f] = sc["Xs"][c], sc["uvs"][c], k, pc.K_of(sc["K4s"][c])
    return X, uv, Ks, counts


@pytest.mark.parametrize("per_rig", [False, True], ids=["shared", "per_rig"])
def test_rig_form(pose_mod, per_rig):
    scs, C = rig_runs(per_rig), 3
    X, uv, Ks, counts = pack_rigs(scs, C)
    E = np.stack([sc["E"] for sc in scs]) if per_rig else scs[0]["E"]
    Xd, uvd, Kd, count = dev(X), dev(uv), dev(Ks), dev(counts, torch.int32)
    rig, per = pose_mod.solve_pnp_ransac_rig(Xd, uvd, Kd, E, C, count, iterations=ITERS, seed=7)
    assert host(rig["result"])[:, 0].tolist() == [1, 1]
    m, p12 = host(per["inliers"]), pose12_of(rig["R"], rig["t"])
    assert not m[1].any() and not m[4].any()                                                # the camera without rows, the unusable one
    for sigma_px in (None, 1.0):
        cov, info, stat = pose_mod.pose_covariance_rig(Xd, uvd, Kd, E, C, (rig["R"], rig["t"]), rig["result"], per["inliers"], sigma_px=sigma_px,
                                                       count=count)
        again = pose_mod.pose_covariance_rig(Xd, uvd, Kd, E, C, (rig["R"], rig["t"]), rig["result"], per["inliers"], sigma_px=sigma_px,
                                             count=count)
        assert torch.equal(cov, again[0]) and torch.equal(info, again[1]) and torch.equal(stat, again[2])
        assert tuple(cov.shape) == (2, 6, 6) and tuple(stat.shape) == (2, 4)
        for s, sc in enumerate(scs):
            masks = [m[s * C + c, :len(sc["Xs"][c])] for c in range(C)]
            ref = pc.covariance(p12[s], host(rig["result"][s]), pc.rig_cams(sc["Xs"], sc["uvs"], sc["K4s"], sc["E"], masks), sigma_px)
            assert ref["stat"][0] == 1 and ref["n"] == int(rig["result"][s, 1])
            check((host(cov[s]), host(info[s]), host(stat[s])), ref, sigma_px, "rig %d sigma=%s per_rig=%s" % (s, sigma_px, per_rig))
            for c in range(C):                                                               # the covariance of camera c's own pose
                got = pose_mod.transport_covariance(cov[s], sc["E"][c])
                want = pc.transport(host(cov[s]), sc["E"][c])
                dg = np.sqrt(np.diag(want))
                assert got.is_cuda and torch.equal(got, got.T) and (np.abs(host(got) - want) <= 1e-12 * dg[:, None] * dg[None, :]).all(), (s, c)


def test_rig_of_one_camera_is_the_frame_form(pose_mod):
    X, uv = np.zeros((2, R_CAP, 3), np.float32), np.zeros((2, R_CAP, 2), np.float32)
    counts = (37, 70)
    for f, n in enumerate(counts):
        X[f], uv[f], _ = pc.frame_scene(300 + f, n, R_CAP, 0.3, K4=batch_K4(f))
    Ks = np.stack([pc.K_of(batch_K4(f)) for f in range(2)]).astype(np.float32)
    Xd, uvd, Kd, count = dev(X), dev(uv), dev(Ks), torch.tensor(counts, dtype=torch.int32, device=DEV)
    res, R, t, mask = pose_mod.solve_pnp_ransac_batch(Xd, uvd, Kd, count, iterations=ITERS, seed=9)
    assert host(res)[:, 0].tolist() == [1, 1]
    frame = pose_mod.pose_covariance_batch(Xd, uvd, Kd, (R, t), res, mask, count=count)
    rig = pose_mod.pose_covariance_rig(Xd, uvd, Kd, rr.IDENTITY_E[None], 1, (R, t), res, mask, count=count)
    m, p12 = host(mask), pose12_of(R, t)
    for f, n in enumerate(counts):
        cam = pc.frame_cam(X[f, :n].astype(np.float64), uv[f, :n].astype(np.float64), batch_K4(f), m[f, :n])
        ref = pc.covariance(p12[f], host(res[f]), [cam])
        for k, name in enumerate(("cov", "info")):
            assert (np.abs(host(rig[k][f]) - host(frame[k][f])) <= pc.bound_matrix(ref, ref[name])).all(), (f, name)
        assert torch.equal(rig[2][f, :2], frame[2][f, :2])


# ------------------------------------------------------------------------------------------------ 5. NEES
def test_nees_kernel(pose_mod):
    trials = pc.calibration_scene()
    B, n = len(trials), pc.CAL_N
    X, uv = np.stack([tr[0] for tr in trials]).astype(np.float32), np.stack([tr[1] for tr in trials]).astype(np.float32)
    P_gt = np.stack([rr.pose_matrix(*tr[2]) for tr in trials])
    Ks = np.repeat(pc.K_of(pc.CAL_K4)[None], B, 0).astype(np.float32)
    Xd, uvd, Kd = dev(X), dev(uv), dev(Ks)
    res, R, t, mask = pose_mod.solve_pnp_ransac_batch(Xd, uvd, Kd, iterations=ITERS, seed=1)
    res = res.clone()
    res[5, 0] = 0                                                                            # a body without a covariance
    cov, info, stat = pose_mod.pose_covariance_batch(Xd, uvd, Kd, (R, t), res, mask)
    p12, m, st, inf_ = pose12_of(R, t), host(mask), host(stat), host(info)
    assert st[:, 0].tolist() == [0.0 if f == 5 else 1.0 for f in range(B)]
    got64 = host(pose_mod.pose_nees((R, t), torch.from_numpy(P_gt), info, stat))
    got32 = host(pose_mod.pose_nees(torch.from_numpy(p12.astype(np.float32)).to(DEV), torch.from_numpy(P_gt.astype(np.float32)).to(DEV), info, stat))
    assert got64.dtype == np.float64 and got64.shape == (B,)
    assert np.isnan(got64).tolist() == [f == 5 for f in range(B)] and np.isnan(got32).tolist() == [f == 5 for f in range(B)]
    for f in range(B):
        if f == 5:
            continue
        ref = pc.covariance(p12[f], host(res[f]), [pc.frame_cam(X[f].astype(np.float64), uv[f].astype(np.float64), pc.CAL_K4, m[f])])
        b = pc.bound_matrix(ref, ref["info"])
        for got, gt in ((got64[f], P_gt[f]), (got32[f], P_gt[f].astype(np.float32).astype(np.float64))):
            e = np.abs(pc.tangent_error(p12[f], gt))
            want = pc.nees(p12[f], gt, ref["info"], ref["stat"])
            bound = float(e @ b @ e)                                                         # the info bound times |e|^2, entry by entry
            note("nees", np.array(abs(got - want)), np.array(bound))
            assert abs(got - want) <= bound, (f, got, want, bound)
            assert abs(got - pc.nees(p12[f], gt, inf_[f], st[f])) <= bound                   # and on the device's own matrix
    print("\nmean NEES on the device over %d frames: %.3f" % (B - 1, float(np.nanmean(got64))))


# ------------------------------------------------------------------------------------------------ 6. pose tail, serving
def tail_K(B):
    return torch.from_numpy(np.stack([np.array([[300.0 + 4 * f, 0, 256.0], [0, 296.0 + 2 * f, 80.0 + f], [0, 0, 1.0]]) for f in range(B)]).astype(np.float32)).to(DEV)


def snapshot(h):
    return ([[t.clone() for t in out] for out in h["out_tuples"]] + [h["pose"][k].clone() for k in ("result", "R", "t", "inliers")]
            + ([h["rig_pose"][k].clone() for k in ("result", "R", "t")] if "rig_pose" in h else []))


def flat(snap):
    return [t for part in snap for t in (part if isinstance(part, list) else [part])]


def test_pose_tail(model, pose_mod):
    """forward_async(pose_K=, pose_cov=): the handle's matrices are the stand-alone batch call on the handle's operands, nothing else
    moves, a replay reproduces the bits, and pose_cov without pose_K is refused"""
    from cofii2p_amd._lib import CofiError

    _, rep, img = rig_inputs()
    B, iters, seed = img.shape[0], 1000, 11
    Ks = tail_K(B)
    model.enable_graphs(True)
    try:
        h0 = model.forward_async(14, rep, img, pose_K=Ks, pose_iterations=iters, pose_seed=seed)
        h0["out_tuples"] = model.finish(h0)
        assert set(h0["pose"]) == {"result", "R", "t", "inliers"}
        plain = flat(snapshot(h0))
        snaps = []
        for sigma_px, kw in ((None, True), (None, True), (2.0, 2.0)):      # the second submission only replays the slot's graph
            h = model.forward_async(14, rep, img, pose_K=Ks, pose_iterations=iters, pose_seed=seed, pose_cov=kw)
            h["out_tuples"] = model.finish(h)
            p, o0 = h["pose"], h["out"][0]
            assert set(p) == {"result", "R", "t", "inliers", "cov", "info", "cov_stat"}
            assert all(torch.equal(a, b) for a, b in zip(flat(snapshot(h)), plain))          # every other output: bit-equal
            want = pose_mod.pose_covariance_batch(o0["coarse_pts_all"], o0["fine_xy_all"], Ks, (p["R"], p["t"]), p["result"], p["inliers"],
                                                  sigma_px=sigma_px, count=o0["count_all"][:, 0], coord_major=True)
            torch.cuda.synchronize()
            assert tuple(p["cov"].shape) == (B, 6, 6) and tuple(p["cov_stat"].shape) == (B, 4)
            for a, b in zip((p["cov"], p["info"], p["cov_stat"]), want):
                assert torch.equal(a, b)
            assert bool((p["cov_stat"][:, 0] <= p["result"][:, 0]).all()) and float(p["cov_stat"][:, 0].sum()) >= 1
            snaps.append([p[k].clone() for k in ("cov", "info", "cov_stat")])
        assert all(torch.equal(a, b) for a, b in zip(snaps[0], snaps[1]))
        assert torch.equal(snaps[2][1], snaps[0][1]) is False and torch.equal(snaps[2][2][:, 1:3], snaps[0][2][:, 1:3])
        for bad in (dict(pose_cov=True), dict(pose_K=Ks, pose_cov=0.0), dict(pose_K=Ks, pose_cov=float("nan"))):
            with pytest.raises(CofiError):
                model.forward_async(14, rep, img, **bad)
        h = model.forward_async(14, rep, img, pose_K=Ks, pose_iterations=iters, pose_seed=seed)   # the slot stays usable, and plain
        h["out_tuples"] = model.finish(h)
        assert set(h["pose"]) == {"result", "R", "t", "inliers"} and all(torch.equal(a, b) for a, b in zip(flat(snapshot(h)), plain))
    finally:
        model.enable_graphs(False)


def test_rig_pose_tail(model, pose_mod):
    """with cameras=3 and rig_extrinsics: handle["rig_pose"] carries the rig call's matrices, handle["pose"] the frame form of every image"""
    rig_in, _, img = rig_inputs()
    B, iters, seed = img.shape[0], 1000, 11
    Ks, E = tail_K(B), rr.rig_extrinsics_around(CAMERAS, np.random.default_rng(77))
    model.enable_graphs(True)
    try:
        h0 = model.forward_async(15, rig_in, img, cameras=CAMERAS, pose_K=Ks, pose_iterations=iters, pose_seed=seed, rig_extrinsics=E)
        h0["out_tuples"] = model.finish(h0)
        plain = flat(snapshot(h0))
        assert "cov" not in h0["rig_pose"] and "cov" not in h0["pose"]
        snaps = []
        for _ in range(2):
            h = model.forward_async(15, rig_in, img, cameras=CAMERAS, pose_K=Ks, pose_iterations=iters, pose_seed=seed, rig_extrinsics=E,
                                    pose_cov=True)
            h["out_tuples"] = model.finish(h)
            assert all(torch.equal(a, b) for a, b in zip(flat(snapshot(h)), plain))
            p, r, o0 = h["pose"], h["rig_pose"], h["out"][0]
            ops_ = (o0["coarse_pts_all"], o0["fine_xy_all"], Ks)
            want = pose_mod.pose_covariance_rig(*ops_, E, CAMERAS, (r["R"], r["t"]), r["result"], p["inliers"], count=o0["count_all"][:, 0],
                                                coord_major=True)
            per = pose_mod.pose_covariance_batch(*ops_, (p["R"], p["t"]), p["result"], p["inliers"], count=o0["count_all"][:, 0], coord_major=True)
            torch.cuda.synchronize()
            assert tuple(r["cov"].shape) == (B // CAMERAS, 6, 6) and tuple(p["cov"].shape) == (B, 6, 6)
            for a, b in zip((r["cov"], r["info"], r["cov_stat"], p["cov"], p["info"], p["cov_stat"]), want + per):
                assert torch.equal(a, b)
            assert bool((r["cov_stat"][:, 0] <= r["result"][:, 0]).all()) and float(r["cov_stat"][:, 0].sum()) >= 1
            snaps.append([t.clone() for t in (r["cov"], r["info"], r["cov_stat"], p["cov"], p["info"], p["cov_stat"])])
        assert all(torch.equal(a, b) for a, b in zip(*snaps))
    finally:
        model.enable_graphs(False)


def test_frame_batcher_covariance(model, pose_mod):
    """FrameBatcher(pose=True, covariance=True): per ticket the matrices of its image and of its rig, as the stand-alone calls give them
    on the stack's own outputs"""
    from cofii2p_amd.serving import FrameBatcher

    C, B, iters = 3, 6, 500
    E = rr.rig_extrinsics_around(C, np.random.default_rng(77))
    imgs = torch.cat([image(i) for i in (40, 41, 42)])
    Ks = np.stack([np.array([[310.0 + 3 * c, 0, 250.0 + c], [0, 305.0, 82.0], [0, 0, 1.0]]) for c in range(C)])
    model.enable_graphs(True)
    try:
        with pytest.raises(ValueError):
            FrameBatcher(model, batch=B, cameras=C, covariance=True)                         # no pose
        fb = FrameBatcher(model, batch=B, cameras=C, streams=1, ring=2, slot_base=90, pose=True, pose_iterations=iters, rig_extrinsics=E,
                          covariance=True, sigma_px=1.5)
        tickets = fb.submit_rig(cloud(31), imgs, K=Ks)
        got = [fb.covariance_result(tk) for tk in tickets]                                   # the first call flushes the half-filled stack
        rig_got = [fb.rig_covariance_result(tk) for tk in tickets]
        j = tickets[0][0]
        st_ = fb._stacks[j]
        h = model.forward_async(96, st_.pyr, st_.img, cameras=C, inputs_stable=True)
        model.finish(h)
        o0, p, r = h["out"][0], fb._poses[j], fb._rig_poses[j]
        ops_ = (o0["coarse_pts_all"], o0["fine_xy_all"], fb._K[j])
        per = pose_mod.pose_covariance_batch(*ops_, (p["R"], p["t"]), p["result"], p["inliers"], sigma_px=1.5, count=o0["count_all"][:, 0],
                                             coord_major=True)
        rig = pose_mod.pose_covariance_rig(*ops_, E, C, (r["R"], r["t"]), r["result"], p["inliers"], sigma_px=1.5, count=o0["count_all"][:, 0],
                                           coord_major=True)
        torch.cuda.synchronize()
        for c, tk in enumerate(tickets):
            assert tuple(got[c][0].shape) == (6, 6) and tuple(got[c][2].shape) == (4,)
            assert all(torch.equal(a, b[tk[2]]) for a, b in zip(got[c], per)), c
            assert all(torch.equal(a, b[0]) for a, b in zip(rig_got[c], rig)), c
        assert float(rig_got[0][2][0]) <= float(fb.rig_pose_result(tickets[0])[0][0])
        with pytest.raises(RuntimeError):
            FrameBatcher(model, batch=B, cameras=C, pose=True).covariance_result((0, 0, 0))
    finally:
        model.enable_graphs(False)


# ------------------------------------------------------------------------------------------------ argument checks
def test_argument_checks(pose_mod):
    from cofii2p_amd import _lib, ops

    lib = _lib.load()
    s = ops._stream()
    assert lib.cofi_pose_covariance(None, None, None, 4, 1.0, 1.0, 0.0, 0.0, None, None, None, 0.0, None, None, None, s) == _lib.COFI_EINVAL
    assert lib.cofi_pose_covariance_batch(None, 12, None, 8, 0, None, 0, None, 4, 1, None, None, None, 0.0, None, None, None, s) == _lib.COFI_EINVAL
    assert lib.cofi_pose_covariance_rig(None, 12, None, 8, 0, None, 0, None, None, 0, 4, 1, 1, None, None, None, 0.0, None, None, None,
                                        s) == _lib.COFI_EINVAL
    assert lib.cofi_pose_nees(None, None, 1, None, None, 4, None, s) == _lib.COFI_EINVAL
    X, uv, _ = pc.frame_scene(1, 20, 20, 0.0)
    Xd, uvd = dev(X), dev(uv)
    K = pc.K_of(pc.FRAME_K4)
    res, R, t, mask = pose_mod.solve_pnp_ransac(Xd, uvd, K, iterations=64)
    p = torch.cat([R.reshape(9), t])
    d = lambda *shape: torch.empty(shape, dtype=torch.float64, device=DEV)  # noqa: E731
    a = lambda t_: ops._p(t_)  # noqa: E731
    outs = (d(6, 6), d(6, 6), d(4))
    good = [a(Xd), a(uvd), None, 20, 700.0, 690.0, 256.0, 80.0, a(p), a(res), a(mask), 0.0, a(outs[0]), a(outs[1]), a(outs[2]), s]
    assert lib.cofi_pose_covariance(*good) == 0
    for i, v in ((3, 0), (4, 0.0), (5, -1.0), (8, None), (11, float("nan")), (12, None), (14, None)):
        bad = list(good)
        bad[i] = v
        assert lib.cofi_pose_covariance(*bad) == _lib.COFI_EINVAL, i
    torch.cuda.synchronize()
    E = _lib.CofiError
    with pytest.raises(E):
        pose_mod.pose_covariance(Xd, uvd, K, (R, t), res, mask, sigma_px=-1.0)
    with pytest.raises(E):
        pose_mod.pose_covariance(Xd, uvd, K, (R, t), res, mask[:10])
    with pytest.raises(E):
        pose_mod.pose_covariance_batch(Xd[None], uvd[None], K[None], p[None], res[None].to(torch.int64), mask[None])
    with pytest.raises(E):
        pose_mod.pose_covariance_batch_into(Xd[None], uvd[None], K[None], None, p[None], res[None], mask[None], d(1, 6, 6), d(1, 6, 6), d(1, 3))
    with pytest.raises(E):
        pose_mod.pose_covariance_rig(Xd[None], uvd[None], K[None], rr.IDENTITY_E[None], 2, p[None], res[None], mask[None])
    with pytest.raises(E):
        pose_mod.pose_nees(p[None], np.eye(4)[None], d(1, 6, 6), d(2, 4))
    with pytest.raises(E):
        pose_mod.pose_nees(p[None], np.eye(3)[None], d(1, 6, 6), d(1, 4))
