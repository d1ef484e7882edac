"""Sub-pixel fine matches on the GPU: cofi_fine_refine against its float64 restatement (tests/fine_refine_refs.py), its borders, its
degenerate similarities and its reproducibility; forward_async(subpixel=True), the pose tail and FrameBatcher on top of it; and poses
from planted scenes.

The tolerance is derived, not tuned.  The operands are the float32 values the kernel reads, so only arithmetic separates the kernel from
the reference.  A cosine of C channels is three fp32 sums of C terms, two square roots, a product and a quotient: relative error below
(C + 8) 2^-24 =: eps whatever the summation order, and |cosine| <= 1, so |peak - ref| <= eps.  The offset 0.5 (s- - s+) / den has a
numerator off by at most eps and a denominator off by at most 4 eps, with |offset| <= 0.5: |delta - ref| <= (eps + 0.5 * 4 eps) / |den|
to first order - 4 eps / |den| with room for the second order once |den| >= 64 eps, which is where a case is compared -, plus 2^-22
towards the rounding of column + delta to fp32.  (That rounding is up to 2^-21 in columns 8 .. 11; |den| <= 4 leaves the first term at
least eps >= 9 * 2^-24, so the bound covers it everywhere on these maps.)"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import fine_refine_refs as fr
import pnp_oracle as po
import rig_pose_refs as rr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CAP, SENT = 80, -77.25
H2, W2 = 8, 12
CS = (1, 3, 4, 63, 64, 65, 128, 130)
COUNTS = (0, 1, 63, 64, 65)


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


def padded(a, ld):
    """a (rows, C) float32 -> a device view of the same values with leading dimension ld"""
    buf = torch.full((a.shape[0], ld), 9.5, dtype=torch.float32, device=DEV)   # the padding is never read: finite, but not 0
    buf[:, :a.shape[1]] = dev(a)
    return buf[:, :a.shape[1]]


def planted_case(C, cap=CAP, h2=H2, w2=W2, seed=0, ell=1.0):
    """cap matches on an h2 x w2 map of planted features: true positions anywhere on the map (border cells included), the patch that
    holds the cell chosen at random among the four that do on each axis.  Everything already rounded to float32."""
    rng = np.random.default_rng(977 * C + 31 * cap + seed)
    basis = fr.C1_BASIS if C == 1 else fr.fourier_basis(C, ell, rng)
    fmap = fr.feature_map(h2, w2, basis).astype(np.float32)
    uv = np.stack([rng.uniform(-0.5, w2 - 0.5, cap), rng.uniform(-0.5, h2 - 0.5, cap)], 1)
    cell = np.clip(np.floor(uv + 0.5), 0, [w2 - 1, h2 - 1])
    w, r = rng.integers(0, 4, cap), rng.integers(0, 4, cap)
    xy = np.stack([(cell[:, 0] - w + 2) / 4.0, (cell[:, 1] - r + 2) / 4.0]).astype(np.float32)   # quarters: exact, left = cell - w
    best = (r * 4 + w).astype(np.int32)
    desc = fr.features(uv, basis).astype(np.float32)
    return {"fmap": fmap, "xy": xy, "best": best, "desc": desc, "cell": cell.T.astype(np.int64), "C": C, "H2": h2, "W2": w2}


def launch(fmap, h2, w2, xy, desc, best, count, frames=1, cs=4.0):
    """cofi_fine_refine itself, into buffers pre-filled with a sentinel -> (sub_xy, peak) device tensors"""
    from cofii2p_amd import _lib, ops

    lib = _lib.load()
    cap = best.numel() // frames
    lead = () if frames == 1 else (frames,)
    sub = torch.full(lead + (2, cap), SENT, dtype=torch.float32, device=DEV)
    peak = torch.full(lead + (cap,), SENT, dtype=torch.float32, device=DEV)
    pc = desc.reshape(frames * cap, -1) if desc.dim() == 3 else desc
    rc = lib.cofi_fine_refine(ops._p(fmap), ops._ld(fmap), fmap.shape[1], h2, w2, ops._p(xy), xy.stride(-2), ctypes.c_float(cs), ops._p(pc),
                              ops._ld(pc), ops._p(best), ops._p(count), cap, ops._p(sub), ops._p(peak), frames, ops._stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return sub, peak


def count_t(*n):
    """count_dev as match_finish leaves it: [matches, threshold index] per frame - (2,) for one frame, (frames, 2) for several"""
    t = torch.tensor([[v, 0] for v in n], dtype=torch.int32, device=DEV)
    return t[0] if len(n) == 1 else t


def run_case(case, count, ldf=None, ldp=None):
    C = case["C"]
    fmap = padded(case["fmap"], ldf) if ldf else dev(case["fmap"])
    desc = padded(case["desc"], ldp) if ldp else dev(case["desc"])
    sub, peak = launch(fmap, case["H2"], case["W2"], dev(case["xy"]), desc, dev(case["best"], torch.int32), count_t(count))
    assert fmap.shape[1] == C
    return sub.cpu().numpy(), peak.cpu().numpy()


def compare(case, count, sub, peak, tag):
    """-> (matches compared, matches left out, largest error / bound).  Asserts the bounds of the module docstring."""
    C, cap = case["C"], len(case["best"])
    ref = fr.fine_refine_ref(case["fmap"], case["H2"], case["W2"], case["xy"], case["desc"], case["best"], count, 4.0)
    eps = (C + 8) * 2.0 ** -24
    assert np.all(sub[:, count:] == SENT) and np.all(peak[count:] == SENT), tag          # rows at or beyond the count: not written
    assert np.isfinite(sub[:, :count]).all() and np.isfinite(peak[:count]).all(), tag
    worst, used, left = 0.0, 0, 0
    for i in range(count):
        cell = case["cell"][:, i]
        den = ref["den"][:, i]
        refined = ~np.isnan(den)
        if np.any(np.abs(den[refined]) < 64 * eps):
            left += 1
            continue
        used += 1
        e = abs(float(peak[i]) - ref["peak"][i])
        assert e <= eps, (tag, i, "peak", e, eps)
        worst = max(worst, e / eps)
        for ax in range(2):
            d, dref = float(sub[ax, i]) - cell[ax], ref["sub_xy"][ax, i] - cell[ax]
            if not refined[ax]:
                assert d == 0.0 and dref == 0.0, (tag, i, ax)                               # a border cell: that axis stays put
                continue
            bound = 4 * eps / abs(den[ax]) + 2.0 ** -22
            assert abs(d - dref) <= bound, (tag, i, ax, d, dref, den[ax], bound)
            worst = max(worst, abs(d - dref) / bound)
    return used, left, worst


# ------------------------------------------------------------------------------------------------ 1. the kernel against the reference
@functools.lru_cache(maxsize=None)
def sweep():
    """every (C, count) once: {(C, count): (used, left out, worst error / bound)}"""
    out = {}
    for C in CS:
        case = planted_case(C)
        for count in COUNTS:
            sub, peak = run_case(case, count)
            out[(C, count)] = compare(case, count, sub, peak, (C, count))
    return out


@pytest.mark.parametrize("C", CS)
def test_kernel_equals_the_reference(C):
    for count in COUNTS:
        used, left, worst = sweep()[(C, count)]
        assert used + left == count
        print("C %3d count %2d: %2d compared, %d left out, largest error / bound %.3f" % (C, count, used, left, worst))


def test_few_cases_are_left_out():
    res = sweep()
    used, left = sum(v[0] for v in res.values()), sum(v[1] for v in res.values())
    worst = max(v[2] for v in res.values())
    print("%d matches compared, %d left out (|den| < 64 eps); largest error / bound %.3f" % (used, left, worst))
    assert used > 0 and left <= 0.01 * (used + left)


@pytest.mark.parametrize("C,ldf,ldp", [(64, 68, 72), (64, 65, 64), (64, 64, 67), (63, 64, 64), (130, 132, 136), (3, 8, 4), (1, 4, 4)])
def test_leading_dimensions(C, ldf, ldp):
    """ldf > C and ldp > C, with and without 16-byte rows: the reference's values, and the very bits of the packed layout"""
    case = planted_case(C, seed=3)
    sub, peak = run_case(case, 65, ldf=ldf, ldp=ldp)
    used, left, worst = compare(case, 65, sub, peak, (C, ldf, ldp))
    assert used >= 60
    sub0, peak0 = run_case(case, 65)
    assert np.array_equal(sub, sub0) and np.array_equal(peak, peak0)     # 16-byte and 4-byte loads sum the same channels in the same order


def stacked_case(C=64, counts=(65, 0, 17), ldf=None, ldp=None):
    cases = [planted_case(C, seed=10 + f) for f in range(len(counts))]
    cat = lambda k, ax=0: np.concatenate([c[k] for c in cases], ax)
    fmap = padded(cat("fmap"), ldf) if ldf else dev(cat("fmap"))
    desc = padded(cat("desc"), ldp) if ldp else dev(cat("desc"))
    xy = dev(np.stack([c["xy"] for c in cases]))
    best = dev(np.stack([c["best"] for c in cases]), torch.int32)
    return cases, fmap, desc, xy, best, count_t(*counts)


@pytest.mark.parametrize("ldf,ldp", [(None, None), (72, 68), (67, 65)])
def test_three_frames_with_three_counts(ldf, ldp):
    counts = (65, 0, 17)
    cases, fmap, desc, xy, best, cnt = stacked_case(64, counts, ldf, ldp)
    sub, peak = launch(fmap, H2, W2, xy, desc, best, cnt, frames=3)
    assert tuple(sub.shape) == (3, 2, CAP) and tuple(peak.shape) == (3, CAP)
    again = launch(fmap, H2, W2, xy, desc, best, cnt, frames=3)
    assert torch.equal(sub, again[0]) and torch.equal(peak, again[1])                     # two runs: the same bits
    for f, (case, n) in enumerate(zip(cases, counts)):
        used, left, _ = compare(case, n, sub[f].cpu().numpy(), peak[f].cpu().numpy(), ("stack", f))
        assert used + left == n
        # frame f of the stacked call = the single-frame call on its slice, bit for bit
        P = H2 * W2
        one = launch(fmap[f * P:(f + 1) * P], H2, W2, xy[f], desc[f * CAP:(f + 1) * CAP], best[f], cnt[f])
        assert torch.equal(one[0], sub[f]) and torch.equal(one[1], peak[f]), f


def test_ops_wrapper():
    from cofii2p_amd import ops
    from cofii2p_amd._lib import CofiError

    cases, fmap, desc, xy, best, cnt = stacked_case()
    want = launch(fmap, H2, W2, xy, desc, best, cnt, frames=3)
    sub, peak = ops.fine_refine(fmap, H2, W2, xy, desc.reshape(3, CAP, 64), best, cnt, 4.0, frames=3)
    torch.cuda.synchronize()
    for f, n in enumerate((65, 0, 17)):
        assert torch.equal(sub[f, :, :n], want[0][f, :, :n]) and torch.equal(peak[f, :n], want[1][f, :n])
    one = ops.fine_refine(fmap[:H2 * W2], H2, W2, xy[0], desc[:CAP], best[0], cnt[0], 4.0)
    assert tuple(one[0].shape) == (2, CAP) and torch.equal(one[0][:, :65], sub[0, :, :65])
    for bad in (lambda: ops.fine_refine(fmap, H2, W2 + 1, xy, desc, best, cnt, 4.0, frames=3),          # the map has other rows
                lambda: ops.fine_refine(fmap, H2, W2, xy, desc[:, :32], best, cnt, 4.0, frames=3),      # descriptors of another width
                lambda: ops.fine_refine(fmap, H2, W2, xy, desc, best, cnt[:2], 4.0, frames=3),          # two counts for three frames
                lambda: ops.fine_refine(fmap, H2, W2, xy, desc, best.long(), cnt, 4.0, frames=3),
                lambda: ops.fine_refine(fmap, H2, W2, xy[:, :, :40], desc, best, cnt, 4.0, frames=3),   # fewer coordinates than rows
                lambda: ops.fine_refine(fmap.cpu(), H2, W2, xy, desc, best, cnt, 4.0, frames=3),
                lambda: ops.fine_refine(fmap, H2, W2, xy, desc, best, cnt, 4.0, frames=7)):
        with pytest.raises(CofiError):
            bad()


# ------------------------------------------------------------------------------------------------ 2. borders
def one_match(fmap, h2, w2, cell, desc, w=1, r=1, count=1):
    """a single match whose matched cell is `cell` (column, row), reached through patch offset (w, r)"""
    xy = dev(np.array([[(cell[0] - w + 2) / 4.0], [(cell[1] - r + 2) / 4.0]], np.float32))
    best = torch.tensor([r * 4 + w], dtype=torch.int32, device=DEV)
    sub, peak = launch(dev(fmap), h2, w2, xy, dev(np.asarray(desc, np.float32)[None]), best, count_t(count))
    return sub.cpu().numpy()[:, 0], float(peak.cpu()[0])


@pytest.mark.parametrize("h2,w2", [(H2, W2), (4, 4)])
def test_borders(h2, w2):
    rng = np.random.default_rng(h2)
    basis = fr.fourier_basis(64, 1.0, rng)
    fmap = fr.feature_map(h2, w2, basis).astype(np.float32)
    for cell, moves in (((0, 2), (False, True)), ((w2 - 1, 1), (False, True)), ((2, 0), (True, False)), ((1, h2 - 1), (True, False)),
                        ((0, 0), (False, False)), ((w2 - 1, h2 - 1), (False, False)), ((1, 2), (True, True))):
        desc = fr.features(np.array([[cell[0] + 0.3, cell[1] - 0.2]]), basis)[0].astype(np.float32)
        for w, r in ((0, 0), (3, 2)):
            sub, peak = one_match(fmap, h2, w2, cell, desc, w, r)
            case = {"fmap": fmap, "H2": h2, "W2": w2, "C": 64, "cell": np.array([[cell[0]], [cell[1]]]), "desc": desc[None],
                    "xy": np.array([[(cell[0] - w + 2) / 4.0], [(cell[1] - r + 2) / 4.0]], np.float32), "best": np.array([r * 4 + w], np.int32)}
            used, left, _ = compare(case, 1, np.full((2, 1), 0.0) + sub[:, None], np.array([peak]), (cell, w, r))
            assert used == 1
            for ax in range(2):                                                             # zero on the border axis ONLY
                assert (sub[ax] != cell[ax]) == moves[ax], (cell, ax, sub)
    # a patch that hangs over the edge, and a padded cell of it "won": nothing to refine, peak 0
    desc = fr.features(np.array([[0.0, 3.0]]), basis)[0].astype(np.float32)
    for cell in ((-2, 2), (-1, 1), (1, -2), (w2, 2), (2, h2 + 1), (-2, -2)):
        w = 0 if cell[0] < 0 else (3 if cell[0] >= w2 else 1)
        r = 0 if cell[1] < 0 else (3 if cell[1] >= h2 else 1)
        sub, peak = one_match(fmap, h2, w2, cell, desc, w, r)
        assert sub[0] == cell[0] and sub[1] == cell[1] and peak == 0.0, (cell, sub, peak)


# ------------------------------------------------------------------------------------------------ 3. degenerate similarities
def angle_map(angles_x, angles_y=None, C=4):
    """a 3 x 3 map whose centre row (and column) holds unit vectors at the given angles to the descriptor e0: cosine = cos(angle)"""
    vec = lambda a: np.array([np.cos(a), np.sin(a)] + [0.0] * (C - 2))
    fmap = np.zeros((9, C), np.float32)
    for x in range(3):
        fmap[3 + x] = vec(angles_x[x])
    if angles_y is not None:
        assert angles_y[1] == angles_x[1]
        fmap[1], fmap[7] = vec(angles_y[0]), vec(angles_y[2])
    return fmap, np.array([1.0] + [0.0] * (C - 1), np.float32)


def test_degenerate_similarities():
    a = np.arccos
    # three identical vectors along x: den == 0 exactly, delta 0; along y a proper peak at the centre
    fmap, desc = angle_map((0.4, 0.4, 0.4), (0.9, 0.4, 0.9))
    sub, peak = one_match(fmap, 3, 3, (1, 1), desc)
    assert sub[0] == 1.0 and sub[1] == 1.0 and abs(peak - np.cos(0.4)) < 1e-6
    # a strictly rising row: half a cell up, whether concave (clamped) or convex (the sign rule); falling: half a cell down
    for sims, want in (((0.36, 0.70, 0.955), 0.5), ((0.1, 0.2, 0.9), 0.5), ((0.1, 0.5, 0.9), 0.5), ((0.955, 0.70, 0.36), -0.5)):
        fmap, desc = angle_map(tuple(a(s) for s in sims))
        sub, _ = one_match(fmap, 3, 3, (1, 1), desc)
        assert sub[0] == 1.0 + want, (sims, sub)
    # a neighbour larger than the centre with den >= 0: half a cell towards it
    for sims, want in (((0.9, 0.2, 0.1), -0.5), ((0.3, 0.2, 0.8), 0.5), ((0.9, 0.2, 0.9), 0.0)):
        fmap, desc = angle_map(tuple(a(s) for s in sims))
        sub, _ = one_match(fmap, 3, 3, (1, 1), desc)
        assert sub[0] == 1.0 + want, (sims, sub)


def test_zero_descriptor_nan_and_inf():
    case = planted_case(64, seed=5)
    n = 65
    base_sub, base_peak = run_case(case, n)
    # an all-zero descriptor: every similarity 0, nothing moves, and the other matches keep their bits
    z = dict(case, desc=case["desc"].copy())
    z["desc"][7] = 0.0
    sub, peak = run_case(z, n)
    assert np.array_equal(sub[:, 7], case["cell"][:, 7].astype(np.float32)) and peak[7] == 0.0
    keep = np.arange(n) != 7
    assert np.array_equal(sub[:, :n][:, keep], base_sub[:, :n][:, keep]) and np.array_equal(peak[:n][keep], base_peak[:n][keep])
    # NaN / Inf in one map pixel: finite outputs everywhere, matches that do not read the pixel keep their bits
    cx, cy = case["cell"][0, :n], case["cell"][1, :n]
    inner = np.nonzero((cx >= 1) & (cx <= W2 - 2) & (cy >= 1) & (cy <= H2 - 2))[0][0]
    hit = (int(cx[inner]), int(cy[inner]))   # (column, row) of a match's own cell, off the border
    for poison in (np.nan, np.inf, -np.inf):
        p = dict(case, fmap=case["fmap"].copy())
        p["fmap"][hit[1] * W2 + hit[0], 11] = poison
        sub, peak = run_case(p, n)
        assert np.isfinite(sub[:, :n]).all() and np.isfinite(peak[:n]).all(), poison
        reads =((np.abs(cx - hit[0]) <= 1) & (cy == hit[1])) | ((np.abs(cy - hit[1]) <= 1) & (cx == hit[0]))
        assert reads.any() and (~reads).sum() >= n // 2
        assert np.array_equal(sub[:, :n][:, ~reads], base_sub[:, :n][:, ~reads]) and np.array_equal(peak[:n][~reads], base_peak[:n][~reads])
        on = (cx == hit[0]) & (cy == hit[1])
        assert np.all(peak[:n][on] == 0.0) and np.all(sub[0, :n][on] == hit[0]) and np.all(sub[1, :n][on] == hit[1])


# ------------------------------------------------------------------------------------------------ 4. through the model
from test_rig_gpu import Opt, cloud, image  # noqa: E402  (the tiny synthetic model and frames of the rig suite)


@pytest.fixture(scope="module")
def model():
    from cofii2p_amd.network import CoFiI2P

    return CoFiI2P(Opt()).to(DEV)


def stack_K(B):
    return torch.from_numpy(np.stack([np.array([[300.0 + 4 * f, 0, 256.0], [0, 296.0 + 2 * f, 80.0 + f], [0, 0, 1.0]]) for f in range(B)]).astype(np.float32)).to(DEV)


ROWS = {"coarse_pts": 0, "patches": 0, "fine_pc": 0, "fine_best": 0, "sel": 0, "fine_xy": 1, "coarse_xy": 1}   # capacity axis of an output


def snapshot(h, outs):
    """every tensor a submission without the flag hands out, cloned - the capacity-sized ones up to the frame's count: the rows beyond
    it are never written"""
    counts = [max(0, int(v)) for v in h["count_host"][:, 0]]
    snap = {}
    for f, o in enumerate(h["out"]):
        for k, v in o.items():
            if not torch.is_tensor(v):
                continue
            if k in ROWS:
                v = v.narrow(ROWS[k], 0, counts[f])
            elif k in ("coarse_pts_all", "fine_xy_all"):
                v = torch.stack([torch.where(torch.arange(v.shape[-1 if k == "fine_xy_all" else 1], device=v.device).reshape(
                    (1, -1) if k == "fine_xy_all" else (-1, 1)) < n, v[g], torch.zeros_like(v[g])) for g, n in enumerate(counts)])
            snap[("out", f, k)] = v.clone()
    snap.update({("finish", f, i): t.clone() for f, out in enumerate(outs) for i, t in enumerate(out)})
    snap.update({("fine_xy", f): t.clone() for f, t in enumerate(h["fine_xy"])})
    return snap


def assert_refined_outputs(h, B, cap):
    """sub_xy_all is ops.fine_refine on the submission's own outputs, bit for bit; the per-frame entries are its rows"""
    from cofii2p_amd import ops

    o0 = h["out"][0]
    fmap = o0["fine_img_map"]
    h2, w2 = Opt.img_H // 2, Opt.img_W // 2
    assert tuple(fmap.shape) == (B * h2 * w2, 64) and tuple(o0["sub_xy_all"].shape) == (B, 2, cap)
    xy = torch.stack([o["coarse_xy"] for o in h["out"]])
    fpc = torch.stack([o["fine_pc"] for o in h["out"]])
    best = torch.stack([o["fine_best"] for o in h["out"]])
    sub, peak = ops.fine_refine(fmap, h2, w2, xy, fpc, best, o0["count_all"], 4.0, frames=B)
    torch.cuda.synchronize()
    counts = [int(v) for v in o0["count_all"][:, 0].cpu()]
    for f, n in enumerate(counts):
        assert n >= 4
        assert torch.equal(o0["sub_xy_all"][f, :, :n], sub[f, :, :n]), f
        assert torch.equal(h["out"][f]["sub_xy"][:, :n], sub[f, :, :n]) and torch.equal(h["out"][f]["sub_peak"][:n], peak[f, :n]), f
        # the geometric decode: within half a cell of (left + best % 4, top + best // 4), which is not fine_xy's cell
        cells = fr.matched_cells(h["out"][f]["coarse_xy"].cpu().numpy(), best[f, :n].cpu().numpy(), 4.0)
        assert np.all(np.abs(sub[f, :, :n].cpu().numpy() - cells) <= 0.5)
    return counts


def test_forward_async_subpixel_stack_of_three(model):
    from cofii2p_amd import pose
    from cofii2p_amd.network import CoFiI2P

    B, iters, seed = 3, 500, 11
    stacked, imgs = CoFiI2P.stack_frames([cloud(31 + f) for f in range(B)], [image(40 + f) for f in range(B)])
    Ks = stack_K(B)
    model.enable_graphs(True)
    try:
        with pytest.raises(ValueError):
            model.forward_async(90, stacked, imgs, mode="val", subpixel=True)              # refused before anything is enqueued
        assert not any(k[3] == 90 for k in model._graphs)
        h0 = model.forward_async(90, stacked, imgs, pose_K=Ks, pose_iterations=iters, pose_seed=seed)
        plain = snapshot(h0, model.finish(h0))
        pose0 = {k: v.clone() for k, v in h0["pose"].items()}
        keys0 = set(model._graphs)
        assert not any("sub" in k for o in h0["out"] for k in o) and "fine_img_map" not in h0["out"][0]
        for _ in range(2):   # the second submission only replays
            h = model.forward_async(91, stacked, imgs, subpixel=True, pose_K=Ks, pose_iterations=iters, pose_seed=seed)
            got = snapshot(h, model.finish(h))
            cap = h["out"][0]["sel"].shape[0]
            for k, v in plain.items():                                                      # nothing that existed moved
                assert torch.equal(got[k], v), k
            counts = assert_refined_outputs(h, B, cap)
            o0 = h["out"][0]
            want = pose.solve_pnp_ransac_batch(o0["coarse_pts_all"], o0["sub_xy_all"], Ks, o0["count_all"][:, 0], iterations=iters, seed=seed,
                                               coord_major=True)
            torch.cuda.synchronize()
            for name, b in zip(("result", "R", "t", "inliers"), want):
                assert torch.equal(h["pose"][name], b), name
        assert not torch.equal(h["pose"]["t"], pose0["t"])                                 # ... and they are other poses than fine_xy's
        new = set(model._graphs) - keys0
        assert len(new) == 1 and keys0 <= set(model._graphs) and "subpixel" in next(iter(new))   # its own recording; the old keys as they were
        # the default call again: its recording, its outputs and its poses are what they were
        h1 = model.forward_async(90, stacked, imgs, pose_K=Ks, pose_iterations=iters, pose_seed=seed)
        again = snapshot(h1, model.finish(h1))
        assert set(again) == set(plain) and all(torch.equal(again[k], v) for k, v in plain.items())
        assert all(torch.equal(h1["pose"][k], v) for k, v in pose0.items())
        # covariance and evaluation monitors: they read the refined points without a switch of their own
        from cofii2p_amd import evaluation

        table = evaluation.EvalTable(B, device=DEV)
        P_gt = torch.eye(4, dtype=torch.float64, device=DEV).repeat(B, 1, 1).contiguous()
        ri = torch.arange(B, dtype=torch.int32, device=DEV)
        h = model.forward_async(91, stacked, imgs, subpixel=True, pose_K=Ks, pose_iterations=iters, pose_seed=seed, pose_cov=True,
                                eval_into=(table, P_gt, ri))
        model.finish(h)
        o0 = h["out"][0]
        cov = pose.pose_covariance_batch(o0["coarse_pts_all"], o0["sub_xy_all"], Ks, (h["pose"]["R"], h["pose"]["t"]), h["pose"]["result"],
                                         h["pose"]["inliers"], count=o0["count_all"][:, 0], coord_major=True)
        want_rows = evaluation.EvalTable(B, device=DEV)
        evaluation.eval_monitors({"object_points": o0["coarse_pts_all"], "image_points": o0["sub_xy_all"], "coord_major": True,
                                  "count": o0["count_all"][:, 0], "pose": (h["pose"]["R"], h["pose"]["t"]), "result": h["pose"]["result"]},
                                 Ks, P_gt, want_rows)
        torch.cuda.synchronize()
        assert torch.equal(h["pose"]["cov"], cov[0]) and torch.equal(h["pose"]["cov_stat"], cov[2])
        assert torch.equal(torch.nan_to_num(table.rows, nan=-1.0), torch.nan_to_num(want_rows.rows, nan=-1.0))   # NaN: RTE / RRE of a failed pose
        assert not bool(torch.isnan(table.rows[:, :3]).any())
    finally:
        model.enable_graphs(False)


def test_forward_async_subpixel_rig_of_two_cameras(model):
    from cofii2p_amd import pose
    from cofii2p_amd.network import CoFiI2P

    C, iters, seed = 2, 500, 5
    rig_in, imgs = CoFiI2P.stack_frames([cloud(31)], [image(40), image(41)])
    Ks, E = stack_K(C), rr.rig_extrinsics_around(C, np.random.default_rng(77))
    model.enable_graphs(True)
    try:
        h0 = model.forward_async(92, rig_in, imgs, cameras=C)
        plain = snapshot(h0, model.finish(h0))
        h = model.forward_async(93, rig_in, imgs, cameras=C, subpixel=True, pose_K=Ks, pose_iterations=iters, pose_seed=seed, rig_extrinsics=E)
        got = snapshot(h, model.finish(h))
        for k, v in plain.items():
            assert torch.equal(got[k], v), k
        assert_refined_outputs(h, C, h["out"][0]["sel"].shape[0])
        o0 = h["out"][0]
        rig, per = pose.solve_pnp_ransac_rig(o0["coarse_pts_all"], o0["sub_xy_all"], Ks, E, C, o0["count_all"][:, 0], iterations=iters, seed=seed,
                                             coord_major=True)
        torch.cuda.synchronize()
        for name in ("result", "R", "t"):
            assert torch.equal(h["rig_pose"][name], rig[name]), name
        for name in ("result", "R", "t", "inliers"):
            assert torch.equal(h["pose"][name], per[name]), name
    finally:
        model.enable_graphs(False)


def test_frame_batcher_subpixel(model):
    from cofii2p_amd import pose
    from cofii2p_amd.network import CoFiI2P
    from cofii2p_amd.serving import FrameBatcher

    B, iters = 3, 400
    frames = [(cloud(31 + f), image(40 + f)) for f in range(B)]
    Ks = [np.array([[310.0 + 3 * i, 0, 250.0 + i], [0, 305.0, 82.0], [0, 0, 1.0]]) for i in range(B)]
    model.enable_graphs(True)
    try:
        stacked, imgs = CoFiI2P.stack_frames([f[0] for f in frames], [f[1] for f in frames])
        h = model.forward_async(94, stacked, imgs, subpixel=True)
        model.finish(h)
        direct = [h["out"][f]["sub_xy"].clone() for f in range(B)]
        fb = FrameBatcher(model, batch=B, streams=1, ring=2, slot_base=95, subpixel=True, pose=True, pose_iterations=iters)
        tickets = [fb.submit(pyr, img, K=Ks[i]) for i, (pyr, img) in enumerate(frames)]
        for i in (2, 0, 1):
            out = fb.result(tickets[i])
            n = out[7].shape[0]
            sxy = fb.sub_xy(tickets[i])
            assert tuple(sxy.shape) == (2, n) and torch.equal(sxy, direct[i][:, :n]), i     # the rows the direct submission has
            assert tuple(fb.fine_xy(tickets[i]).shape) == (2, n) and not torch.equal(fb.fine_xy(tickets[i]), sxy)
            res, R, t, inl = fb.pose_result(tickets[i])                                     # pose=True: the pose of the sub-pixel points
            want = pose.solve_pnp_ransac(out[7].contiguous(), sxy.t().contiguous(), Ks[i], iterations=iters, seed=tickets[i][2])
            assert torch.equal(res.cpu(), want[0].cpu()) and torch.equal(R, want[1]) and torch.equal(t, want[2]) and torch.equal(inl, want[3]), i
        with pytest.raises(RuntimeError):
            FrameBatcher(model, batch=B, slot_base=99).sub_xy(tickets[0])
    finally:
        model.enable_graphs(False)


# ------------------------------------------------------------------------------------------------ 5. planted scenes: the pose gains
@pytest.mark.parametrize("seed", fr.POSE_SEEDS)
def test_planted_scene_pose(seed):
    from cofii2p_amd import ops, pose

    sc = fr.planted_scene(seed, 1.0)
    n, h2, w2 = len(sc["X"]), sc["H2"], sc["W2"]
    fmap, desc, xy, X = dev(sc["fmap"]), dev(sc["desc"]), dev(sc["coarse_xy"]), dev(sc["X"])
    cnt = count_t(n)
    patches = ops.extract_patches_nhwc(fmap, h2, w2, xy, cnt, n, 4.0)
    _, best = ops.fine_match(patches, desc, xy, cnt, 4.0)
    sub, peak = ops.fine_refine(fmap, h2, w2, xy, desc, best, cnt, 4.0)
    torch.cuda.synchronize()
    hard = dev(fr.matched_cells(sc["coarse_xy"], best.cpu().numpy(), 4.0).astype(np.float64))
    assert float((sub - hard).abs().max()) <= 0.5
    fx, fy, cx, cy = sc["K4"]
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])
    err = []
    for pts in (hard, sub):
        res, R, t, _ = pose.solve_pnp_ransac(X, pts.t().contiguous(), K, iterations=256, seed=3)
        assert int(res[0]) == 1 and int(res[1]) >= n - n // 8                              # no outliers were planted
        err.append(float(np.linalg.norm(t.cpu().numpy().astype(np.float64) - sc["t"])))
    rms = [float(np.sqrt(np.mean((p.t().cpu().numpy() - sc["uv"]) ** 2))) for p in (hard, sub)]
    print("seed %d: %.3f -> %.3f cells rms per axis, translation error %.4f -> %.4f m" % (seed, rms[0], rms[1], err[0], err[1]))
    assert err[1] < err[0]
