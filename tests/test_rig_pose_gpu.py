"""The rig solver (cofi_pnp_ransac_rig: ONE pose per rig from the matches of all its cameras) stage by stage against the float64
restatement tests/rig_pose_refs.py, its edges, and its way up through forward_async(rig_extrinsics=...) and FrameBatcher.

The pattern is that of tests/test_pose_stages_gpu.py: the workspace is filled with bytes 0xFF before the call, so a slab row the kernel
did not write reads as all-sentinel; outputs are poisoned; the slab is found through pose.pnp_rig_workspace_views; everything is
compared as numpy.  The slab holds RIG poses.  The scenes (rig_pose_refs.SCENES / GPU_RUNS: S = 2 rigs of C = 1, 2, 3, 4 or 6 cameras,
capacity 128, 512 hypotheses) are the ones tests/test_rig_pose_refs_cpu.py admits as well conditioned."""
import types

import numpy as np
import pytest
import torch

import pnp_oracle as po
import rig_pose_refs as rr
import test_pose_stages_gpu as st
from test_pose_stages_gpu import BAND, FAIL, IDENTITY, SENTINEL, THR2, ULP1, bits, has_pose
from test_rig_gpu import CAMERAS, model, rig_inputs  # noqa: F401  (model: the fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED, ITERS, CAP = rr.SEED, rr.ITERS, 128


@pytest.fixture(scope="module")
def pose_mod():
    from cofii2p_amd import pose
    return pose


def K_of(K4):
    return np.array([[K4[0], 0, K4[2]], [0, K4[1], K4[3]], [0, 0, 1.0]], np.float32)


def pack(names, cap=CAP, fill_seed=0, fill=None):
    """the rigs `names` (equal C) in buffers of capacity cap: X (B,cap,3), uv (B,cap,2) with finite junk (or `fill`) behind the counts,
    counts (B,), Ks (B,3,3), E (S,C,3,4) float32"""
    scs = [rr.scene(n) for n in names]
    C = len(scs[0]["counts"])
    assert all(len(sc["counts"]) == C for sc in scs)
    rng = np.random.default_rng(fill_seed)
    B = len(scs) * C
    X, uv = st.junk(rng, (B, cap, 3), 50.0), st.junk(rng, (B, cap, 2), 512.0)
    if fill is not None:
        X[:], uv[:] = fill, fill
    counts, Ks = [], []
    for s, sc in enumerate(scs):
        for c in range(C):
            n = sc["counts"][c]
            X[s * C + c, :n], uv[s * C + c, :n] = sc["Xs"][c], sc["uvs"][c]
            counts.append(n)
            Ks.append(K_of(sc["K4s"][c]))
    return X, uv, counts, np.stack(Ks), np.stack([sc["E"] for sc in scs]).astype(np.float32), C


def run_rig(pose_mod, X, uv, Ks, E, C, count=None, iterations=ITERS, seed=SEED, refine_iters=20, coord_major=False, pad=0, short=0):
    """one call of solve_pnp_ransac_rig_into into a sentinel-filled workspace (over-allocated by `pad` bytes, or `short` bytes too small)
    and poisoned outputs; everything comes back as numpy"""
    X, uv = np.ascontiguousarray(X, np.float32), np.ascontiguousarray(uv, np.float32)
    B, cap = X.shape[:2]
    S = B // C
    dev = lambda a: torch.from_numpy(np.array(a, order="C")).to(DEV)
    need = pose_mod.pnp_rig_workspace(iterations, S)
    ws = torch.full((need + pad - short,), 0xFF, dtype=torch.uint8, device=DEV)
    rig_pose = torch.full((S, 12), float("nan"), dtype=torch.float32, device=DEV)
    rig_result = torch.full((S, 3), -99, dtype=torch.int32, device=DEV)
    pose = torch.full((B, 12), float("nan"), dtype=torch.float32, device=DEV)
    result = torch.full((B, 3), -99, dtype=torch.int32, device=DEV)
    mask = torch.full((B, cap), 0xEE, dtype=torch.uint8, device=DEV)
    cnt = None if count is None else torch.tensor(list(count), dtype=torch.int32, device=DEV)
    pose_mod.solve_pnp_ransac_rig_into(dev(X), dev(uv.transpose(0, 2, 1) if coord_major else uv), dev(Ks), dev(np.asarray(E, np.float32)), C, cnt,
                                       ws, rig_pose, rig_result, pose, result, mask, iterations=iterations, seed=seed,
                                       refine_iters=refine_iters, coord_major=coord_major)
    keys, slab = pose_mod.pnp_rig_workspace_views(ws, iterations, S)
    assert keys.shape == (S,) and keys.dtype == torch.int64 and slab.shape == (S, iterations, 12) and slab.dtype == torch.float32
    return types.SimpleNamespace(rig_result=rig_result.cpu().numpy(), rig_pose=rig_pose.cpu().numpy(), result=result.cpu().numpy(),
                                 pose=pose.cpu().numpy(), mask=mask.cpu().numpy(), keys=keys.cpu().numpy(), slab=slab.cpu().numpy(),
                                 tail=ws[need:].cpu().numpy(), iterations=iterations, C=C)


_runs = {}


def named_run(pose_mod, run, refine_iters=20):
    """the GPU run `run` of rig_pose_refs.GPU_RUNS, computed once and shared; nobody modifies it"""
    if (run, refine_iters) not in _runs:
        X, uv, counts, Ks, E, C = pack(rr.GPU_RUNS[run])
        _runs[run, refine_iters] = run_rig(pose_mod, X, uv, Ks, E, C, count=counts, refine_iters=refine_iters)
    return _runs[run, refine_iters]


def assert_same_rig(a, sa, b, sb, counts, tag=""):
    """rig sa of run a and rig sb of run b bit for bit: rig outputs, key, slab rows, and every image's result, pose and mask"""
    C = a.C
    assert a.rig_result[sa].tolist() == b.rig_result[sb].tolist(), (tag, a.rig_result[sa].tolist(), b.rig_result[sb].tolist())
    assert np.array_equal(bits(a.rig_pose[sa]), bits(b.rig_pose[sb])), (tag, a.rig_pose[sa], b.rig_pose[sb])
    assert a.keys[sa] == b.keys[sb], tag
    rows = min(a.iterations, b.iterations)
    diff = (bits(a.slab[sa, :rows]) != bits(b.slab[sb, :rows])).any(-1)
    assert not diff.any(), (tag, "slab rows differ", np.nonzero(diff)[0].tolist()[:8])
    for c in range(C):
        fa, fb, n = sa * C + c, sb * C + c, max(0, counts[c])
        assert a.result[fa].tolist() == b.result[fb].tolist(), (tag, c, a.result[fa].tolist(), b.result[fb].tolist())
        assert np.array_equal(bits(a.pose[fa]), bits(b.pose[fb])), (tag, c)
        assert np.array_equal(a.mask[fa, :n], b.mask[fb, :n]), (tag, c)
        assert not a.mask[fa, n:].any() and not b.mask[fb, n:].any(), (tag, c)


def assert_rig_failed(r, s, tag=""):
    """the documented failure output of rig s and of all its images, and nothing written into its slab"""
    assert r.rig_result[s].tolist() == FAIL, (tag, r.rig_result[s].tolist())
    assert np.array_equal(bits(r.rig_pose[s]), bits(IDENTITY)), tag
    assert r.keys[s] == 0 and (bits(r.slab[s]) == SENTINEL).all(), tag
    for f in range(s * r.C, (s + 1) * r.C):
        assert r.result[f].tolist() == FAIL and np.array_equal(bits(r.pose[f]), bits(IDENTITY)) and not r.mask[f].any(), (tag, f)


def pose_of(row):
    p = np.asarray(row, np.float32).astype(np.float64)
    return p[:9].reshape(3, 3), p[9:]


def ulps(got12, R, t):
    """|dR| in float32 ulp of 1, |dt| in ulp of the largest |t| component"""
    g = np.asarray(got12, np.float64)
    return float(np.abs(g[:9] - R.ravel()).max() / ULP1), float(np.abs(g[9:] - t).max() / np.spacing(np.float32(np.abs(t).max())))


# ------------------------------------------------------------------------------------------- C = 1, identity: the batched solver
@pytest.mark.parametrize("names,cap", [(("n500", "n37"), 512), (("n5", "n4"), 64)])
def test_one_camera_with_identity_extrinsics_is_the_batched_solver(pose_mod, names, cap):
    """composing with the identity multiplies by 1 and adds 0: result, keys, masks and every slab row are the batched call's bits; the
    refit runs the rig's Jacobian chain through the identity, 2 float32 ulp"""
    rng = np.random.default_rng(5)
    X, uv = st.junk(rng, (2, cap, 3), 50.0), st.junk(rng, (2, cap, 2), 512.0)
    counts = []
    for f, name in enumerate(names):
        Xs, uvs, _ = st.scene(name)
        X[f, :len(Xs)], uv[f, :len(Xs)] = Xs, uvs
        counts.append(len(Xs))
    want = st.run(pose_mod, X, uv, count=counts)
    E = np.broadcast_to(rr.IDENTITY_E.astype(np.float32), (2, 1, 3, 4))
    got = run_rig(pose_mod, X, uv, np.broadcast_to(st.K.astype(np.float32), (2, 3, 3)), E, 1, count=counts)
    assert want.result[:, 0].tolist() == [1, 1]
    assert np.array_equal(got.result, want.result) and np.array_equal(got.rig_result, want.result)
    assert np.array_equal(got.keys, want.keys) and np.array_equal(got.mask, want.mask)
    assert np.array_equal(bits(got.slab), bits(want.slab))
    assert np.array_equal(bits(got.rig_pose), bits(got.pose))
    for f in range(2):
        dR, dt = ulps(got.pose[f], *pose_of(want.pose[f]))
        print("C = 1 %-5s: refit bit-equal to the batched call: %s (|dR| %.2f ulp, |dt| %.2f ulp)"
              % (names[f], np.array_equal(bits(got.pose[f]), bits(want.pose[f])), dR, dt))
        assert dR <= 2 and dt <= 2, (names[f], dR, dt)


# ------------------------------------------------------------------------------------------- stage 1: hypotheses
@pytest.mark.parametrize("run", sorted(rr.GPU_RUNS))
def test_hypotheses_equal_the_reference(pose_mod, run):
    """every slab row against rig_hypothesis: existence agrees, |dR| <= 4 ulp of 1, |dt| <= 4 ulp of max |t|, for all but at most 0.5 %
    of the hypotheses with a pose on either side (the cap of test_pose_stages_gpu.test_hypotheses_equal_the_oracle)"""
    r = named_run(pose_mod, run)
    for s, name in enumerate(rr.GPU_RUNS[run]):
        slab = r.slab[s]
        dev_has = has_pose(slab)
        either, exceptions, worst_R, worst_t = 0, [], 0.0, 0.0
        for h, ref in enumerate(rr.scene_hypotheses(name, SEED + s)):
            if ref is None and not dev_has[h]:
                continue
            either += 1
            if (ref is None) != (not dev_has[h]):
                exceptions.append("%s hypothesis %d: pose on the %s only" % (name, h, "device" if ref is None else "reference"))
                continue
            bad, dR, dt = rr.stage1_differs(ref, pose_of(slab[h]))
            if bad:
                exceptions.append("%s hypothesis %d: |dR| %.1f ulp, |dt| %.1f ulp" % (name, h, dR / ULP1, dt))
            else:
                worst_R, worst_t = max(worst_R, dR), max(worst_t, dt)
        print("stage 1 %-8s: %d hypotheses with a pose, %d exceptions, worst |dR| %.2f ulp, |dt| %.2f ulp" % (name, either, len(exceptions), worst_R / ULP1, worst_t))
        for e in exceptions:
            print("   exception:", e)
        assert either >= ITERS // 4, (name, either)
        assert len(exceptions) <= 0.005 * either, exceptions


# ------------------------------------------------------------------------------------------- stage 2: consensus and winner
def check_rig_consensus(pose_mod, r, s, sc, tag, counts=None):
    """rig s of run r against the fp64 classification of its own slab rows composed with the extrinsics (each composition rounded once
    to float32, as the kernel scores) -> (lo, hi) total inliers per hypothesis"""
    C = r.C
    counts = list(sc["counts"]) if counts is None else counts
    res = r.rig_result[s].tolist()
    assert res[0] == 1, (tag, res)
    assert list(pose_mod.pnp_decode_key(r.keys[s])) == res[1:3], (tag, res)
    per = r.result[s * C:(s + 1) * C]
    assert per[:, 0].tolist() == [1] * C and per[:, 2].tolist() == [res[2]] * C, (tag, per.tolist())
    assert res[1] == int(per[:, 1].sum()) == int(r.mask[s * C:(s + 1) * C].sum()), (tag, res, per[:, 1].tolist())
    Xs, uvs = [sc["Xs"][c][:counts[c]] for c in range(C)], [sc["uvs"][c][:counts[c]] for c in range(C)]
    lo, hi = np.zeros(r.iterations, int), np.zeros(r.iterations, int)
    rows = has_pose(r.slab[s])
    errs_w = None
    with np.errstate(all="ignore"):
        for h in np.nonzero(rows)[0]:
            errs = rr.rig_score(pose_of(r.slab[s, h]), Xs, uvs, sc["K4s"], sc["E"], f32=True)
            for e in errs:
                if e is not None:
                    lo[h] += int((e <= THR2 * (1 - BAND)).sum())
                    hi[h] += int((e <= THR2 * (1 + BAND)).sum())
            if h == res[2]:
                errs_w = errs
    w = res[2]
    assert 0 <= w < r.iterations and rows[w], (tag, res)
    assert lo[w] <= res[1] <= hi[w], (tag, res, lo[w], hi[w])
    for c in range(C):
        m = r.mask[s * C + c]
        assert int(m.sum()) == per[c, 1] and not m[max(0, counts[c]):].any(), (tag, c)
        if errs_w[c] is None:
            assert per[c, 1] == 0, (tag, c)
            continue
        e = errs_w[c]
        outside = (e <= THR2 * (1 - BAND)) | ~(e <= THR2 * (1 + BAND))
        wrong = outside & (m[:counts[c]].astype(bool) != (e <= THR2))
        assert not wrong.any(), (tag, c, "mask differs from fp64 outside the band at", np.nonzero(wrong)[0].tolist())
    better = np.nonzero(lo > hi[w])[0]
    assert better.size == 0, (tag, "larger consensus sets than the winner's", better.tolist(), res)
    earlier = [h for h in range(w) if lo[h] == hi[h] and lo[h] >= res[1]]
    assert not earlier, (tag, "earlier hypotheses with as many inliers", earlier, res)
    return lo, hi


@pytest.mark.parametrize("run", sorted(rr.GPU_RUNS))
def test_consensus_and_winner(pose_mod, run):
    r = named_run(pose_mod, run)
    for s, name in enumerate(rr.GPU_RUNS[run]):
        lo, hi = check_rig_consensus(pose_mod, r, s, rr.scene(name), name)
        print("stage 2 %-8s: winner %d with %d inliers %s; %d hypotheses have a point inside the band"
              % (name, r.rig_result[s, 2], r.rig_result[s, 1], r.result[s * r.C:(s + 1) * r.C, 1].tolist(), int((lo != hi).sum())))


def test_tie_goes_to_the_lowest_id(pose_mod):
    """noise-free, all inliers, three cameras: many hypotheses reach all 64 rows; the winner is exactly the first of them"""
    r = named_run(pose_mod, "C3clean")
    lo, hi = check_rig_consensus(pose_mod, r, 0, rr.scene("clean"), "clean")
    assert (lo == hi).all()
    full = np.nonzero(lo == 64)[0]
    assert full.size >= 16, full.size
    assert r.rig_result[0].tolist() == [1, 64, int(full[0])] and r.result[:3, 1].tolist() == [30, 20, 14]


# ------------------------------------------------------------------------------------------- stage 3: refit
def rig_cost64(pose12, Xs, uvs, K4s, E):
    R, t = pose_of(pose12)
    return rr.rig_cost_and_normal(R, t, Xs, uvs, K4s, E)[0]


@pytest.mark.parametrize("run", ["C2", "C3", "C4", "C6"])
def test_refit_equals_the_reference(pose_mod, run):
    """refine_iters = 0 returns the winner's slab row as the rig pose; 1, 2, 5 and 20 equal refine_rig from that row on the rows of the
    device's masks within 2 float32 ulp, change poses only and do not raise the fp64 cost; every image's pose is E_c o rig_pose
    recomputed in fp64 within 1 ulp"""
    iters = (0, 1, 2, 5, 20)
    runs = {it: named_run(pose_mod, run, it) for it in iters}
    r0 = runs[0]
    C = r0.C
    for s, name in enumerate(rr.GPU_RUNS[run]):
        sc = rr.scene(name)
        assert r0.rig_result[s, 0] == 1, (name, r0.rig_result[s].tolist())
        w = int(r0.rig_result[s, 2])
        assert np.array_equal(bits(r0.rig_pose[s]), bits(r0.slab[s, w])), (name, r0.rig_pose[s], r0.slab[s, w])
        ms = [r0.mask[s * C + c, :sc["counts"][c]].astype(bool) for c in range(C)]
        Xs, uvs = [sc["Xs"][c][ms[c]] for c in range(C)], [sc["uvs"][c][ms[c]] for c in range(C)]
        start = pose_of(r0.slab[s, w])
        for it in iters:
            r = runs[it]
            for c in range(C):      # the per-image poses are compositions of the float32 rig pose
                dR, dt = ulps(r.pose[s * C + c], *rr.compose(sc["E"][c], pose_of(r.rig_pose[s])))
                assert dR <= 1 and dt <= 1, (name, it, c, dR, dt)
            if it == 0:
                continue
            assert np.array_equal(r.rig_result, r0.rig_result) and np.array_equal(r.result, r0.result) and np.array_equal(r.mask, r0.mask)
            assert np.array_equal(bits(r.slab), bits(r0.slab)) and np.array_equal(r.keys, r0.keys)
            with np.errstate(all="ignore"):
                Rr, tr = rr.refine_rig(start[0], start[1], Xs, uvs, sc["K4s"], sc["E"], it)
            dR, dt = ulps(r.rig_pose[s], Rr, tr)
            print("stage 3 %-8s refine_iters %2d: |dR| %.2f ulp of 1, |dt| %.2f ulp of max |t|" % (name, it, dR, dt))
            assert dR <= 2 and dt <= 2, (name, it, dR, dt)
        c0, c20 = rig_cost64(r0.rig_pose[s], Xs, uvs, sc["K4s"], sc["E"]), rig_cost64(runs[20].rig_pose[s], Xs, uvs, sc["K4s"], sc["E"])
        print("stage 3 %-8s: %d inliers, fp64 cost %.6e -> %.6e" % (name, sum(int(m.sum()) for m in ms), c0, c20))
        assert np.isfinite(c0) and c20 <= c0, (name, c0, c20)


# ------------------------------------------------------------------------------------------- the feature
@pytest.mark.parametrize("run,name,starved", [("C3", "starved", (1, 2)), ("C4", "thin", (0, 1, 2, 3))])
def test_starved_cameras_are_solved_by_the_rig(pose_mod, run, name, starved):
    """What the per-image tail cannot do: the images with too few matches (of the thin rig: ALL images) come back [0, 0, -1] from
    solve_pnp_ransac_batch, while the rig solve succeeds, counts their rows as inliers and lands where the float64 reference lands:
    RTE / RRE against the ground truth no worse than the reference's own plus what 2 float32 ulp of the refit can move them (RTE:
    2 ulp on each of R's entries times |t| plus 2 ulp of max |t| on each component; RRE: 2 ulp on each entry in degrees, three angles,
    doubled for the linearisation)"""
    sc = rr.scene(name)
    X, uv, counts, Ks, E, C = pack(rr.GPU_RUNS[run])
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    res_b = pose_mod.solve_pnp_ransac_batch(dev(X), dev(uv), dev(Ks), count=torch.tensor(counts, dtype=torch.int32, device=DEV),
                                            iterations=ITERS, seed=SEED)[0].cpu().numpy()
    for c in starved:
        assert res_b[c].tolist() == FAIL, (c, res_b[c].tolist())
    rig, per = pose_mod.solve_pnp_ransac_rig(dev(X), dev(uv), dev(Ks), dev(E), C, count=torch.tensor(counts, dtype=torch.int32, device=DEV),
                                             iterations=ITERS, seed=SEED)
    res, inl = rig["result"].cpu().numpy()[0], per["result"].cpu().numpy()[:C, 1]
    with np.errstate(all="ignore"):
        ok, Rr, tr, masks, best, per_ref = rr.solve_rig(sc["Xs"], sc["uvs"], sc["K4s"], sc["E"], iterations=ITERS, seed=SEED, f32=True)
    assert ok and res[0] == 1, (ok, res.tolist())
    print("%s: device winner %d inliers %s; reference winner %d inliers %s" % (name, res[2], inl.tolist(), best, per_ref))
    for c in starved:
        assert inl[c] > 0 and inl[c] == per_ref[c], (c, inl.tolist(), per_ref)
    assert res[1] == int(inl.sum()) >= 11
    Rg, tg = rig["R"].cpu().numpy()[0].astype(np.float64), rig["t"].cpu().numpy()[0].astype(np.float64)
    rte, rre = rr.rig_errors(Rg, tg, sc["T"])
    rte_ref, rre_ref = rr.rig_errors(Rr, tr, sc["T"])
    tmax = float(np.abs(sc["T"][1]).max())
    tol_rte = 2 * ULP1 * 3 * float(np.linalg.norm(sc["T"][1])) + 2 * np.sqrt(3) * float(np.spacing(np.float32(tmax)))
    tol_rre = 2 * 3 * np.degrees(2 * ULP1)
    print("%s: RTE %.6f m (reference %.6f), RRE %.6f deg (reference %.6f)" % (name, rte, rte_ref, rre, rre_ref))
    assert rte <= rte_ref + tol_rte and rre <= rre_ref + tol_rre, (rte, rte_ref, rre, rre_ref)


# ------------------------------------------------------------------------------------------- edges
def test_rig_without_an_eligible_camera_fails_alone(pose_mod):
    """counts 3 / 3 / 3 (nine rows, no camera with four), 0 / -5 / 2, and an unusable camera holding the only four rows: the documented
    failure; the good rig next to each is bit-equal to running alone with seed + 1"""
    X, uv, counts, Ks, E, C = pack(("even", "even"))
    alone = run_rig(pose_mod, X[C:], uv[C:], Ks[C:], E[1:], C, count=counts[C:], seed=SEED + 1)
    assert alone.rig_result[0, 0] == 1
    for bad in ((3, 3, 3), (0, -5, 2)):
        r = run_rig(pose_mod, X, uv, Ks, E, C, count=list(bad) + counts[C:])
        assert_rig_failed(r, 0, str(bad))
        assert_same_rig(r, 1, alone, 0, counts[C:], "the good rig beside %s" % (bad,))
    Kb = Ks.copy()
    Kb[0, 0, 0] = 0.0
    r = run_rig(pose_mod, X, uv, Kb, E, C, count=[30, 3, 2] + counts[C:])
    assert_rig_failed(r, 0, "the only camera with four rows is unusable")
    assert_same_rig(r, 1, alone, 0, counts[C:])
    base = run_rig(pose_mod, X, uv, Ks, E, C, count=counts)
    r = run_rig(pose_mod, X, uv, Ks, E, C, count=counts[:C] + [3, 3, 3])
    assert_rig_failed(r, 1, "the second rig")
    assert_same_rig(r, 0, base, 0, counts[:C], "the good rig before it")


@pytest.mark.parametrize("entry,value", [((0, 0), 0.0), ((1, 1), -700.0)], ids=["fx=0", "fy<0"])
def test_unusable_camera_is_ignored(pose_mod, entry, value):
    """camera 1 of the even rig with fx = 0 or fy < 0: never drawn, never scored - the rig is the one whose camera 1 has no rows, bit for
    bit; its image gets the composed pose with 0 inliers and a zero mask"""
    X, uv, counts, Ks, E, C = pack(("even", "starved"))
    Kb = Ks.copy()
    Kb[1][entry] = value
    r = run_rig(pose_mod, X, uv, Kb, E, C, count=counts)
    empty = run_rig(pose_mod, X, uv, Ks, E, C, count=[counts[0], 0] + counts[2:])
    assert r.rig_result[0, 0] == 1 and r.result[1].tolist() == [1, 0, int(r.rig_result[0, 2])] and not r.mask[1].any()
    assert r.result[0, 1] >= 10 and r.result[2, 1] >= 10
    assert_same_rig(r, 0, empty, 0, [counts[0], 0, counts[2]], "unusable against empty")
    assert_same_rig(r, 1, empty, 1, counts[C:], "the rig beside it")
    dR, dt = ulps(r.pose[1], *rr.compose(rr.scene("even")["E"][1], pose_of(r.rig_pose[0])))
    assert dR <= 1 and dt <= 1
    check_rig_consensus(pose_mod, empty, 0, rr.scene("even"), "camera 1 empty", counts=[counts[0], 0, counts[2]])


def test_camera_without_rows(pose_mod):
    """camera 4 of the six-camera rig has no rows: composed pose, 0 inliers, zero mask, and the rig holds to the reference (stages 1 - 3
    above run on this rig)"""
    r = named_run(pose_mod, "C6")
    sc = rr.scene("six")
    assert sc["counts"][4] == 0 and r.rig_result[0, 0] == 1
    assert r.result[4].tolist() == [1, 0, int(r.rig_result[0, 2])] and not r.mask[4].any()
    dR, dt = ulps(r.pose[4], *rr.compose(sc["E"][4], pose_of(r.rig_pose[0])))
    assert dR <= 1 and dt <= 1 and np.isfinite(r.pose).all()


def test_count_above_capacity_clamps(pose_mod):
    X, uv, counts, Ks, E, C = pack(("even", "even"), cap=30)
    want = run_rig(pose_mod, X, uv, Ks, E, C, count=counts)
    got = run_rig(pose_mod, X, uv, Ks, E, C, count=[31, 1000, 2 ** 31 - 1, 30, 30, 64])
    none = run_rig(pose_mod, X, uv, Ks, E, C, count=None)
    for s in range(2):
        assert_same_rig(got, s, want, s, [30] * 3, "count above capacity")
        assert_same_rig(none, s, want, s, [30] * 3, "no count")
    assert want.rig_result[:, 0].tolist() == [1, 1]


def test_rows_behind_count_are_never_read(pose_mod):
    X, uv, counts, Ks, E, C = pack(rr.GPU_RUNS["C6"])
    Xn, uvn = X.copy(), uv.copy()
    for f, n in enumerate(counts):
        for a in (Xn, uvn):
            a[f, n:] = np.resize(np.array([np.nan, np.inf, -np.inf], np.float32), a[f, n:].shape)
    got = run_rig(pose_mod, Xn, uvn, Ks, E, C, count=counts)
    for s in range(2):
        assert_same_rig(got, s, named_run(pose_mod, "C6"), s, counts[s * C:(s + 1) * C], "NaN / Inf behind count, rig %d" % s)


def test_nan_in_a_valid_row(pose_mod):
    X, uv, counts, Ks, E, C = pack(rr.GPU_RUNS["C3"])
    X, uv = X.copy(), uv.copy()
    X[3 + 1, 7], uv[3 + 1, 7] = np.nan, np.nan          # rig 1 ('even'), camera 1, row 7
    r = run_rig(pose_mod, X, uv, Ks, E, C, count=counts)
    assert r.rig_result[1, 0] == 1 and r.mask[4, 7] == 0
    assert np.isfinite(r.rig_pose).all() and np.isfinite(r.pose).all()
    rows = has_pose(r.slab[1])                            # every row untouched or completely finite
    sc = rr.scene("even")
    rows_el = rr.eligible_rows(sc["counts"], sc["K4s"])
    sampled = np.array([rr.camera_draw(SEED + 1, h, rows_el) == 1 and 7 in po.sample4(SEED + 1, h, 30) for h in range(ITERS)])
    assert sampled.any() and not rows[sampled].any()      # a hypothesis that drew the row has no pose
    assert_same_rig(r, 0, named_run(pose_mod, "C3"), 0, counts[:C], "the rig beside it")


def test_layouts_and_extrinsics_forms_are_bit_equal(pose_mod):
    """point-major against coordinate-major pixels; one set of extrinsics shared by both rigs against the same matrices per rig"""
    X, uv, counts, Ks, E, C = pack(("even", "even"))
    base = run_rig(pose_mod, X, uv, Ks, E, C, count=counts)
    assert np.array_equal(E[0], E[1]) and base.rig_result[:, 0].tolist() == [1, 1]
    for tag, r in (("coordinate-major", run_rig(pose_mod, X, uv, Ks, E, C, count=counts, coord_major=True)),
                   ("shared extrinsics", run_rig(pose_mod, X, uv, Ks, E[0], C, count=counts)),
                   ("4x4 extrinsics", run_rig(pose_mod, X, uv, Ks, np.concatenate([E, np.broadcast_to(np.float32([0, 0, 0, 1]), (2, C, 1, 4))], 2), C, count=counts))):
        for s in range(2):
            assert_same_rig(r, s, base, s, counts[:C], tag)
    assert not np.array_equal(bits(base.rig_pose[0]), bits(base.rig_pose[1]))      # seed + s: the same rig twice is solved twice


def test_iteration_counts_that_fill_no_wave(pose_mod):
    """1, 15, 17 and 100 hypotheses (16 per wave, 64 per workgroup), the workspace over-allocated by 4 KiB"""
    X, uv, counts, Ks, E, C = pack(rr.GPU_RUNS["C3"])
    full = named_run(pose_mod, "C3")
    for it in (1, 15, 17, 100):
        r = run_rig(pose_mod, X, uv, Ks, E, C, count=counts, iterations=it, pad=4096)
        assert r.tail.size == 4096 and (r.tail == 0xFF).all(), (it, "bytes behind the last slab were written")
        for s, name in enumerate(rr.GPU_RUNS["C3"]):
            has_pose(r.slab[s])
            assert np.array_equal(bits(r.slab[s]), bits(full.slab[s, :it])), (it, s)
            if r.rig_result[s, 0] == 1:
                assert 0 <= r.rig_result[s, 2] < it
                check_rig_consensus(pose_mod, r, s, rr.scene(name), "iterations %d rig %d" % (it, s))
            else:
                assert r.rig_result[s].tolist() == FAIL and np.array_equal(bits(r.rig_pose[s]), bits(IDENTITY)) and not r.mask[s * C:(s + 1) * C].any()
        if it == 100:
            assert r.rig_result[:, 0].tolist() == [1, 1]


def test_capacity_on_either_side_of_the_staging_switch(pose_mod):
    """capacity 3276 is the last whose rows fit the 64 KiB the staged form allows itself, 3277 the first that scores from global memory;
    the switch looks at the capacity alone, so the same valid rows reach both forms: bit-equal, and equal to capacity 128"""
    for cap in (3276, 3277):
        X, uv, counts, Ks, E, C = pack(rr.GPU_RUNS["C6"], cap=cap, fill_seed=cap)
        for coord_major in (False, True):
            r = run_rig(pose_mod, X, uv, Ks, E, C, count=counts, coord_major=coord_major)
            for s in range(2):
                assert_same_rig(r, s, named_run(pose_mod, "C6"), s, counts[s * C:(s + 1) * C], "capacity %d coord_major %s rig %d" % (cap, coord_major, s))


def test_workspace_too_small_is_refused(pose_mod):
    from cofii2p_amd._lib import CofiError

    X, uv, counts, Ks, E, C = pack(rr.GPU_RUNS["C3"])
    with pytest.raises(CofiError, match="COFI_EWORKSPACE"):
        run_rig(pose_mod, X, uv, Ks, E, C, count=counts, short=1)
    assert pose_mod.pnp_rig_workspace(ITERS, 2) == pose_mod.pnp_batch_workspace(ITERS, 2) and pose_mod.pnp_rig_workspace(0, 2) == 0


def test_argument_checks(pose_mod):
    from cofii2p_amd._lib import CofiError

    X, uv, counts, Ks, E, C = pack(rr.GPU_RUNS["C3"])
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    Xd, uvd, Kd, Ed = dev(X), dev(uv), dev(Ks), dev(E)
    ok = dict(iterations=16)
    for bad in (lambda: pose_mod.solve_pnp_ransac_rig(Xd, uvd, Kd, Ed, 4, **ok),              # 6 images are no rigs of 4
                lambda: pose_mod.solve_pnp_ransac_rig(Xd, uvd, Kd, Ed, 0, **ok),
                lambda: pose_mod.solve_pnp_ransac_rig(Xd, uvd, Kd, Ed[:, :2], 3, **ok),       # extrinsics of two cameras
                lambda: pose_mod.solve_pnp_ransac_rig(Xd, uvd, Kd, dev(np.stack([E[0]] * 3)), 3, **ok),   # of three rigs
                lambda: pose_mod.solve_pnp_ransac_rig(Xd, uvd, Kd, E * 1.01, 3, **ok),        # a host set that is no rotation
                lambda: pose_mod.solve_pnp_ransac_rig(Xd.double(), uvd, Kd, Ed, 3, **ok),
                lambda: pose_mod.solve_pnp_ransac_rig(Xd, uvd, Kd[:3], Ed, 3, **ok),
                lambda: pose_mod.solve_pnp_ransac_rig(Xd, uvd, Kd, Ed, 3, count=torch.tensor(counts, device=DEV), **ok)):   # int64 counts
        with pytest.raises(CofiError):
            bad()
    rig, per = pose_mod.solve_pnp_ransac_rig(Xd, uvd, Kd, E, 3, **ok)                          # a host set is uploaded
    assert tuple(rig["result"].shape) == (2, 3) and tuple(rig["R"].shape) == (2, 3, 3) and tuple(rig["t"].shape) == (2, 3)
    assert tuple(per["result"].shape) == (6, 3) and tuple(per["R"].shape) == (6, 3, 3) and tuple(per["inliers"].shape) == (6, CAP)


# ------------------------------------------------------------------------------------------- pipeline
def rig_K(B):
    return torch.from_numpy(np.stack([np.array([[300.0 + 4 * f, 0, 256.0], [0, 296.0 + 2 * f, 80.0 + f], [0, 0, 1.0]]) for f in range(B)]).astype(np.float32)).to(DEV)


def pipeline_E():
    return rr.rig_extrinsics_around(CAMERAS, np.random.default_rng(77))


def assert_handle_equals(h, rig, per):
    for name in ("result", "R", "t"):
        assert torch.equal(h["rig_pose"][name], rig[name]), name
    for name in ("result", "R", "t", "inliers"):
        assert torch.equal(h["pose"][name], per[name]), name


def test_rig_pose_tail(model, pose_mod):
    """forward_async(cameras=3, pose_K=, rig_extrinsics=): handle["pose"] and handle["rig_pose"] are solve_pnp_ransac_rig on the
    submission's own outputs, a second submission replays the captured graph with equal results, eval_into writes all B rows, and the
    call without rig_extrinsics is still the batched tail"""
    from cofii2p_amd import evaluation
    from cofii2p_amd._lib import CofiError

    rig_in, rep, img = rig_inputs()
    B, iters, seed = img.shape[0], 1000, 11
    S = B // CAMERAS
    Ks, E = rig_K(B), pipeline_E()
    model.enable_graphs(True)
    try:
        snaps = []
        for _ in range(2):      # the second submission only replays the slot's graph
            h = model.forward_async(12, rig_in, img, cameras=CAMERAS, pose_K=Ks, pose_iterations=iters, pose_seed=seed, rig_extrinsics=E)
            model.finish(h)
            o0 = h["out"][0]
            rig, per = pose_mod.solve_pnp_ransac_rig(o0["coarse_pts_all"], o0["fine_xy_all"], Ks, E, CAMERAS, o0["count_all"][:, 0],
                                                     iterations=iters, seed=seed, coord_major=True)
            torch.cuda.synchronize()
            assert tuple(h["rig_pose"]["result"].shape) == (S, 3) and tuple(h["pose"]["result"].shape) == (B, 3)
            assert_handle_equals(h, rig, per)
            snaps.append([h["rig_pose"][k].clone() for k in ("result", "R", "t")] + [h["pose"][k].clone() for k in ("result", "R", "t", "inliers")])
        assert all(torch.equal(a, b) for a, b in zip(*snaps))
        # per-rig extrinsics holding the same matrices, given as the pair rig_extrinsics returns: read in place
        pair = pose_mod.rig_extrinsics(np.stack([E] * S), CAMERAS, DEV)
        h = model.forward_async(12, rig_in, img, cameras=CAMERAS, pose_K=Ks, pose_iterations=iters, pose_seed=seed, rig_extrinsics=pair)
        model.finish(h)
        assert all(torch.equal(a, b) for a, b in zip(snaps[0], [h["rig_pose"][k] for k in ("result", "R", "t")] + [h["pose"][k] for k in ("result", "R", "t", "inliers")]))
        # the evaluation monitors read handle["pose"]: all B rows are written
        table = evaluation.EvalTable(B, device=DEV)
        P_gt = torch.eye(4, dtype=torch.float64, device=DEV).repeat(B, 1, 1).contiguous()
        ri = torch.arange(B, dtype=torch.int32, device=DEV)
        assert bool(torch.isnan(table.rows).all())
        h = model.forward_async(12, rig_in, img, cameras=CAMERAS, pose_K=Ks, pose_iterations=iters, pose_seed=seed, rig_extrinsics=E,
                                eval_into=(table, P_gt, ri))
        model.finish(h)
        written = (~torch.isnan(table.rows)).any(1)
        assert bool(written.all()), written.tolist()
        # without rig_extrinsics: the batched tail, as tests/test_rig_gpu.py::test_pose_tail_on_a_rig asserts
        h = model.forward_async(12, rig_in, img, cameras=CAMERAS, pose_K=Ks, pose_iterations=iters, pose_seed=seed)
        model.finish(h)
        o0 = h["out"][0]
        want = pose_mod.solve_pnp_ransac_batch(o0["coarse_pts_all"], o0["fine_xy_all"], Ks, o0["count_all"][:, 0], iterations=iters, seed=seed,
                                               coord_major=True)
        torch.cuda.synchronize()
        assert "rig_pose" not in h
        for a, b in zip((h["pose"]["result"], h["pose"]["R"], h["pose"]["t"], h["pose"]["inliers"]), want):
            assert torch.equal(a, b)
        # refusals, before anything is enqueued: the slot stays usable
        for kwargs in (dict(cameras=CAMERAS, rig_extrinsics=E),                                  # no pose_K
                       dict(cameras=CAMERAS, pose_K=Ks, rig_extrinsics=E[:2]),                   # extrinsics of two cameras
                       dict(cameras=CAMERAS, pose_K=Ks, rig_extrinsics=E * 1.01),                # no rotations
                       dict(cameras=CAMERAS, pose_K=Ks, rig_extrinsics=np.stack([E] * 3))):      # of three rigs
            with pytest.raises(CofiError):
                model.forward_async(12, rig_in, img, **kwargs)
        with pytest.raises(CofiError):
            model.forward_async(12, rep, img, pose_K=Ks, rig_extrinsics=E[:1])                   # cameras == 1
        h = model.forward_async(12, rig_in, img, cameras=CAMERAS, pose_K=Ks, pose_iterations=iters, pose_seed=seed, rig_extrinsics=E)
        model.finish(h)
        assert all(torch.equal(a, b) for a, b in zip(snaps[0][:3], [h["rig_pose"][k] for k in ("result", "R", "t")]))
    finally:
        model.enable_graphs(False)


def test_frame_batcher_rig_pose(model, pose_mod):
    """FrameBatcher(cameras=3, pose=True, rig_extrinsics=E): the three tickets of a rig share one rig pose, which is the direct call on
    the stack's outputs; pose_result stays per image; a partly filled stack is padded with a copy of its last rig; per-rig extrinsics
    given to submit_rig fill the stack's buffer"""
    from cofii2p_amd.serving import FrameBatcher
    from test_rig_gpu import cloud, image

    C, B, iters = 3, 6, 500
    E = pipeline_E()
    imgs = torch.cat([image(i) for i in (40, 41, 42)])
    Ks = np.stack([np.array([[310.0 + 3 * c, 0, 250.0 + c], [0, 305.0, 82.0], [0, 0, 1.0]]) for c in range(C)])
    model.enable_graphs(True)
    try:
        with pytest.raises(ValueError):
            FrameBatcher(model, batch=B, cameras=C, rig_extrinsics=E)                # no pose
        with pytest.raises(ValueError):
            FrameBatcher(model, batch=B, cameras=1, pose=True, rig_extrinsics=E[:1])
        outs = {}
        for mode, slot_base in (("shared", 60), ("per_rig", 70)):
            fb = FrameBatcher(model, batch=B, cameras=C, streams=1, ring=2, slot_base=slot_base, pose=True, pose_iterations=iters,
                              rig_extrinsics=E if mode == "shared" else "per_rig")
            if mode == "shared":
                with pytest.raises(ValueError):
                    fb.submit_rig(cloud(31), imgs, K=Ks, extrinsics=E)
                tickets = fb.submit_rig(cloud(31), imgs, K=Ks)
            else:
                with pytest.raises(ValueError):
                    fb.submit_rig(cloud(31), imgs, K=Ks)
                tickets = fb.submit_rig(cloud(31), imgs, K=Ks, extrinsics=E)
            got = [fb.rig_pose_result(tk) for tk in tickets]                         # the first call flushes the half-filled stack
            for g in got[1:]:
                assert all(torch.equal(a, b) for a, b in zip(g, got[0]))
            j = tickets[0][0]
            st_ = fb._stacks[j]
            h = model.forward_async(80, st_.pyr, st_.img, cameras=C, inputs_stable=True)
            model.finish(h)
            o0 = h["out"][0]
            rig, per = pose_mod.solve_pnp_ransac_rig(o0["coarse_pts_all"], o0["fine_xy_all"], fb._K[j], E, C, o0["count_all"][:, 0],
                                                     iterations=iters, seed=0, coord_major=True)
            torch.cuda.synchronize()
            assert torch.equal(got[0][0], rig["result"][0]) and torch.equal(got[0][1], rig["R"][0]) and torch.equal(got[0][2], rig["t"][0])
            for c, tk in enumerate(tickets):                                         # per image, as before
                res, R, t, inl = fb.pose_result(tk)
                assert torch.equal(res, per["result"][c]) and torch.equal(R, per["R"][c]) and torch.equal(t, per["t"][c])
                assert torch.equal(inl, per["inliers"][c, :inl.shape[0]]) and int(res[2]) == int(got[0][0][2])
            pad = fb._rig_poses[j]                                                   # the padding rig: the same rig under seed 1
            assert pad["result"].shape[0] == B // C and torch.equal(pad["result"][1], rig["result"][1])
            outs[mode] = [t.clone() for t in got[0]]
        assert all(torch.equal(a, b) for a, b in zip(outs["shared"], outs["per_rig"]))
        with pytest.raises(RuntimeError):
            FrameBatcher(model, batch=B, cameras=C, pose=True).rig_pose_result((0, 0, 0))
    finally:
        model.enable_graphs(False)
