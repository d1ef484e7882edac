"""The SORTED KPConv aggregation kernels (cofi_kpconv_aggregate_rec_sorted, cofi_kpconv_aggregate_c4_sorted, cofi_kpconv_fused_rec_sorted:
record gathers for the sorted prefix of a neighbour row only, flags from the bit table of cofi_kp_pack_bits) against the unsorted kernels,
bit for bit, on index tables that keep the promise - rows as the KNN kernel emits them (ops.knn), some cut short by a shadow tail.  No test
feeds an unsorted table to the sorted form: the promise is the contract, a broken promise is undefined.
Needs a real MI355X:  python -m pytest tests -m gpu"""
import itertools

import numpy as np
import pytest
import torch

import kpconv_prefix_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SIGMA = 0.35
HS = (4, 12, 16, 20, 64, 100, 128)
GEOMETRIES = ("mixed", "dense", "empty", "boundary", "far", "ties")
FLAGS = ("mixed", "zeros", "ones")


@pytest.fixture(scope="module")
def ops():
    from cofii2p_amd import ops as _ops

    assert torch.cuda.is_available()
    saved, _ops.GEMM_MODE = _ops.GEMM_MODE, "f32"
    yield _ops
    _ops.GEMM_MODE = saved


def G(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _kernel_points(g):
    return g.uniform(-0.3, 0.3, (15, 3)).astype(np.float32)


def _dirs(g, n):
    d = g.standard_normal((n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def _points(g, kind, frames, M, N, rs):
    """-> q_pts (frames * M, 3), s_pts (frames * N, 3): the geometries of tests/test_kpconv_prefix_cpu.py around per-frame centres"""
    qs, ss = [], []
    for f in range(frames):
        centre = np.array([0.3 + f, -0.2, 0.1]) + (np.array([4000.0, -7000.0, 900.0]) if kind == "far" else 0.0)
        if kind == "dense":      # every support point inside every query's support
            s, q = centre + _dirs(g, N) * g.uniform(0, 0.3 * rs, (N, 1)), centre + _dirs(g, M) * g.uniform(0, 0.3 * rs, (M, 1))
        elif kind == "empty":    # nothing inside
            s, q = centre + _dirs(g, N) * g.uniform(3 * rs, 5 * rs, (N, 1)), centre + _dirs(g, M) * g.uniform(0, 0.5 * rs, (M, 1))
        elif kind == "boundary":   # shells within 1e-6 relative of the support radius around one spot, the queries all but on it
            rel = g.choice([-1e-6, -1e-7, 0.0, 1e-7, 1e-6], N)
            rel[::4] = g.uniform(-0.9, 2.0, len(rel[::4]))
            s, q = centre + _dirs(g, N) * ((1.0 + rel) * rs)[:, None], centre + _dirs(g, M) * g.uniform(0, 1e-6 * rs, (M, 1))
        elif kind == "ties":     # a few points drawn with replacement; the queries are support points
            pool = centre + _dirs(g, 12) * g.uniform(0, 1.5 * rs, (12, 1))
            s = pool[g.integers(0, 12, N)]
            q = s[g.integers(0, N, M)]
        else:                    # "mixed", "far": a cube a few support radii wide
            s, q = centre + g.uniform(-2 * rs, 2 * rs, (N, 3)), centre + g.uniform(-2 * rs, 2 * rs, (M, 3))
        qs.append(q)
        ss.append(s)
    return np.concatenate(qs).astype(np.float32), np.concatenate(ss).astype(np.float32)


def _tables(ops, g, q_pts, s_pts, frames, H, tails):
    """frame-local (frames * M, H) int32 rows as the KNN kernel emits them: ascending canonical distance, N behind the last support row;
    tails: rows cut short at a random length (0 .. H), the rest shadow entries - still a sorted row"""
    M, N = q_pts.shape[0] // frames, s_pts.shape[0] // frames
    idx = torch.cat([ops.knn(s_pts[f * N:(f + 1) * N].contiguous(), q_pts[f * M:(f + 1) * M].contiguous(), H) for f in range(frames)], 0)
    idx = idx.cpu().numpy()
    assert idx.shape == (frames * M, H) and ((idx >= 0) & (idx <= N)).all()
    assert (np.diff((idx == N).astype(np.int8), axis=1) >= 0).all()   # shadow entries only behind the valid ones
    if tails:
        cut = g.integers(0, H + 1, idx.shape[0])
        cut[::3] = H
        idx[np.arange(H)[None, :] >= cut[:, None]] = N
    return G(idx.astype(np.int32))


def _feats(g, rows, C, flags):
    f = g.standard_normal((rows, C)).astype(np.float32)
    if flags == "zeros":
        f = -np.abs(f)           # every row sums to < 0: all flags 0, npos 0, cnt 1 - whatever lies inside the support
    elif flags == "ones":
        f = np.abs(f) + 0.01     # all flags 1: npos = the row's valid entries, far more than lie inside the support
    else:
        f[::5] = 0
    return G(f)


def _cases(g, frames):
    """every H with every geometry; sizes, flags, processing order and shadow tails cycle through their values alongside"""
    sizes = [(8, 40), (64, 300), (64, 40), (8, 300)]
    extras = [(False, False), (True, True), (True, False), (False, True)]
    for (hi, H), (ki, kind) in itertools.product(enumerate(HS), enumerate(GEOMETRIES)):
        (M, N), fl, (order, tails) = sizes[(hi + ki) % 4], FLAGS[(hi + ki) % 3], extras[(2 * hi + ki) % 4]
        yield H, kind, M, N, fl, order, tails


def _run_twice(fn):
    a = fn()
    b = fn()
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    return a


# C -> kernel form: 4 c4, 32 <2,1>, 64 <4,1>, 128 <4,2>
@pytest.mark.parametrize("frames", [1, 3])
@pytest.mark.parametrize("C", [4, 32, 64, 128])
def test_sorted_equals_unsorted(ops, monkeypatch, C, frames):
    monkeypatch.setenv("COFI_KPCONV_RECORDS", "1")
    monkeypatch.setenv("COFI_KPCONV_PREFIX", "1")
    g = np.random.default_rng(100 * C + frames)
    kp = _kernel_points(g)
    rs = float(np.sqrt((kp.astype(np.float64) ** 2).sum(1)).max()) + SIGMA
    seen = {"nin_gt_npos": False, "npos_gt_nin": False, "any_inside": False}
    for H, kind, M, N, fl, with_order, tails in _cases(g, frames):
        q_np, s_np = _points(g, kind, frames, M, N, rs)
        q_pts, s_pts = G(q_np), G(s_np)
        idx = _tables(ops, g, q_pts, s_pts, frames, H, tails)
        feats = _feats(g, frames * N, C, fl)
        order = G(np.concatenate([g.permutation(M) for _ in range(frames)]).astype(np.int32)) if with_order else None
        for planes in ((False,) if C == 4 else (False, True)):
            def run(srt):
                agg, cnt = ops.kpconv_aggregate(feats, q_pts, s_pts, idx, G(kp), SIGMA, frames=frames, order=order, planes=planes, sorted_tables=srt)
                return (agg.planes if isinstance(agg, ops.SplitA) else agg), cnt

            a0, c0 = run(False)
            a1, c1 = _run_twice(lambda: run(True))
            what = (C, frames, H, kind, M, N, fl, with_order, tails, planes)
            assert a0.dtype == a1.dtype and a0.shape == a1.shape and torch.equal(a0, a1), what   # planes: hi and lo in one tensor
            assert torch.equal(c0, c1), what
            # what the case exercises, on the host: survivors and flags per row
            if not planes:
                Mf = M
                nin = np.zeros(frames * M, dtype=np.int64)
                ix = idx.cpu().numpy()
                for f in range(frames):
                    sp = np.concatenate([s_np[f * N:(f + 1) * N], np.full((1, 3), 1e9, dtype=np.float32)])
                    d2 = R.kernel_d2(q_np[f * Mf:(f + 1) * Mf], sp[ix[f * Mf:(f + 1) * Mf]])
                    nin[f * Mf:(f + 1) * Mf] = ((d2 < R.support_radius2(kp, SIGMA)) & (ix[f * Mf:(f + 1) * Mf] < N)).sum(1)
                npos = np.where(c1.cpu().numpy() > 1, c1.cpu().numpy(), 0)
                seen["any_inside"] |= bool((nin > 0).any()) and float(a1.abs().max()) > 0
                seen["nin_gt_npos"] |= bool((nin > npos + 1).any())
                seen["npos_gt_nin"] |= bool((npos > nin).any())
                if kind == "dense" and not tails:
                    assert (nin == min(H, N)).all(), what
                if kind == "empty":
                    assert (nin == 0).all() and float(a1.abs().max()) == 0.0, what
    assert all(seen.values()), seen   # npos differs from nin in both directions, and the support is not empty throughout


def test_env_switch_forces_the_unsorted_kernels(ops, monkeypatch):
    """COFI_KPCONV_PREFIX=0: no bit table is written, the promise is ignored"""
    g = np.random.default_rng(9)
    kp = _kernel_points(g)
    q_np, s_np = _points(g, "mixed", 1, 8, 40, 0.8)
    q_pts, s_pts = G(q_np), G(s_np)
    idx = _tables(ops, g, q_pts, s_pts, 1, 20, False)
    feats = _feats(g, 40, 32, "mixed")
    calls = []
    real = ops.kp_pack_bits
    monkeypatch.setattr(ops, "kp_pack_bits", lambda *a, **k: calls.append(1) or real(*a, **k))
    out = {}
    for env in ("1", "0"):
        monkeypatch.setenv("COFI_KPCONV_PREFIX", env)
        n0 = len(calls)
        out[env] = ops.kpconv_aggregate(feats, q_pts, s_pts, idx, G(kp), SIGMA, sorted_tables=True)
        assert len(calls) - n0 == (1 if env == "1" else 0)
    assert torch.equal(out["1"][0], out["0"][0]) and torch.equal(out["1"][1], out["0"][1])


@pytest.mark.parametrize("frames", [1, 3])
@pytest.mark.parametrize("C", [32, 64])
def test_fused_sorted_equals_unsorted(ops, monkeypatch, C, frames):
    """cofi_kpconv_fused_rec_sorted against cofi_kpconv_fused_rec on y and the statistics partials (32 channels: 128 neighbours per
    phase; 64 channels: 64, the second phase is the third chunk)"""
    monkeypatch.setattr(ops, "GEMM_MODE", "bf16x3")
    monkeypatch.setenv("COFI_KPCONV_RECORDS", "1")
    monkeypatch.setenv("COFI_KPCONV_PREFIX", "1")
    g = np.random.default_rng(7 * C + frames)
    kp = _kernel_points(g)
    rs = float(np.sqrt((kp.astype(np.float64) ** 2).sum(1)).max()) + SIGMA
    w = ops.presplit(G((g.standard_normal((C, 15 * C)) * 0.1).astype(np.float32)))
    b = G(g.standard_normal(C).astype(np.float32))
    M = 64
    assert ops.kpconv_fused_slab_rows(C, M, frames) > 0
    sizes, flags, extras = itertools.cycle([40, 300]), itertools.cycle(FLAGS), itertools.cycle([(False, False), (True, True), (True, False), (False, True)])
    nonzero = False
    for H, kind in itertools.product(HS, GEOMETRIES):
        N, fl, (with_order, tails) = next(sizes), next(flags), next(extras)
        q_np, s_np = _points(g, kind, frames, M, N, rs)
        q_pts, s_pts = G(q_np), G(s_np)
        idx = _tables(ops, g, q_pts, s_pts, frames, H, tails)
        feats = _feats(g, frames * N, C, fl)
        order = G(np.concatenate([g.permutation(M) for _ in range(frames)]).astype(np.int32)) if with_order else None

        def run(srt):
            y, part, _ = ops.kpconv_fused(feats, q_pts, s_pts, idx, G(kp), SIGMA, w, b, stat_width=1, frames=frames, order=order, sorted_tables=srt)
            return y, part

        y0, p0 = run(False)
        y1, p1 = _run_twice(lambda: run(True))
        assert torch.equal(y0, y1) and torch.equal(p0, p1), (C, frames, H, kind, N, fl, with_order, tails)
        assert bool(torch.isfinite(y1).all())
        nonzero |= float((y1 - b).abs().max()) > 0
    assert nonzero


@pytest.mark.parametrize("frames", [1, 3])
@pytest.mark.parametrize("N", [1, 31, 32, 33, 63, 64, 65, 100, 300])
def test_bit_table_equals_row_pos(ops, N, frames):
    """cofi_kp_pack_bits on support records (stride 4) and first-layer records (stride 8) against row_sum_positive, per frame"""
    g = np.random.default_rng(N + 1000 * frames)
    for C, fill in ((32, "mixed"), (4, "mixed"), (32, "zeros"), (4, "ones")):
        feats = _feats(g, frames * N, C, fill)
        pts = G(g.standard_normal((frames * N, 3)).astype(np.float32))
        row_pos = ops.row_sum_positive(feats).cpu().numpy().reshape(frames, N)
        want = R.pack_bits(row_pos)
        recs = ops.kp_pack_support(feats, pts)
        bits = ops.kp_pack_bits(recs, frames)
        assert bits.shape == want.shape and bits.dtype == torch.int32
        assert (bits.cpu().numpy().view(np.uint32) == want).all(), (N, frames, C, fill)
        if C == 4:   # the first layer's 32-byte records: the flag is the record's last float
            recs8 = torch.cat([feats, recs], 1).contiguous()
            assert (ops.kp_pack_bits(recs8, frames).cpu().numpy().view(np.uint32) == want).all()
        assert fill != "mixed" or N < 31 or (0 < row_pos.sum() < row_pos.size)


class Opt:
    img_H, img_W, img_fine_resolution_scale, norm = 160, 512, 32, "gn"


def test_stack_forward_with_and_without_the_promise(monkeypatch):
    """a 2-frame stack-mode forward in the flagship arithmetic: the pyramid key "sorted_tables" (build_pyramid sets it, stack_frames keeps
    it) routes every routed KPConv layer to the sorted kernels; the same input without the key runs the unsorted ones - identical outputs"""
    from cofii2p_amd import ops
    from cofii2p_amd.network import CoFiI2P
    from cofii2p_amd.preprocess import build_pyramid
    from cofii2p_amd.synth import make_frame, subsample_indices

    monkeypatch.setenv("COFI_KPCONV_RECORDS", "1")
    monkeypatch.setenv("COFI_KPCONV_PREFIX", "1")
    pyrs, imgs = [], []
    for fid in (31, 32):
        fr = make_frame(fid, 4096)
        sub = [torch.from_numpy(s).to(DEV) for s in subsample_indices(4096, 5, seed=fid)]
        pyr = build_pyramid(torch.from_numpy(fr.points).to(DEV), sub)
        pyr["feats"] = torch.from_numpy(fr.feats).to(DEV)
        assert pyr["sorted_tables"] is True
        pyrs.append(pyr)
        imgs.append(torch.from_numpy(fr.img)[None].to(DEV))
    stacked, img = CoFiI2P.stack_frames(pyrs, imgs)
    assert stacked.get("sorted_tables") is True
    plain = {k: v for k, v in stacked.items() if k != "sorted_tables"}
    assert "sorted_tables" not in CoFiI2P.stack_frames([pyrs[0], {k: v for k, v in pyrs[1].items() if k != "sorted_tables"}], imgs)[0]
    calls = []
    real = ops.kp_pack_bits
    monkeypatch.setattr(ops, "kp_pack_bits", lambda *a, **k: calls.append(1) or real(*a, **k))
    model = CoFiI2P(Opt(), arithmetic="bf16x6").to(DEV).eval()
    got = model.finish(model.forward_async(3, stacked, img))
    assert len(calls) > 0   # the sorted kernels ran (warm-up and capture)
    n = len(calls)
    ref = model.finish(model.forward_async(4, plain, img))
    assert len(calls) == n  # and not without the promise
    assert len(got) == 2
    for f in range(2):
        for i in range(8):
            assert torch.equal(got[f][i], ref[f][i]), (f, i)
