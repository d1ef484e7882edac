"""KPConv aggregation from 16-byte support records (cofi_kpconv_aggregate_rec, cofi_kp_pack_support, the records the GroupNorm apply
kernels emit) and the step loop sized to the support: the records path against the COFI_KPCONV_RECORDS=0 path bit for bit, chosen
neighbour counts in the support against an fp64 evaluation of kpconv.py:91-116, the flags behind `cnt`, and one residual block with
records on and off.
Needs a real MI355X:  python -m pytest tests -m gpu"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SIGMA = 0.35


@pytest.fixture(scope="module")
def ops():
    from cofii2p_amd import ops as _ops

    assert torch.cuda.is_available()
    saved, _ops.GEMM_MODE = _ops.GEMM_MODE, "f32"
    yield _ops
    _ops.GEMM_MODE = saved


def G(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
    if dtype is not None:
        t = t.to(dtype)
    return t.to(DEV)


def _kernel_points(g):
    return g.uniform(-0.3, 0.3, (15, 3)).astype(np.float32)


def _rsup(kp):
    return float(np.sqrt((kp.astype(np.float64) ** 2).sum(1)).max()) + SIGMA


def _aggregate(ops, monkeypatch, records, *args, **kw):
    monkeypatch.setenv("COFI_KPCONV_RECORDS", "1" if records else "0")
    agg, cnt = ops.kpconv_aggregate(*args, **kw)
    if isinstance(agg, ops.SplitA):
        agg = agg.planes
    torch.cuda.synchronize()
    return agg, cnt


def _random_case(g, frames, M, N, H, C, strided):
    """Stack-mode operands: points in a cube a few support radii wide (a part of every row lies inside the support), random indices
    with shadows (idx == N), rows of zeros among the features."""
    kp = _kernel_points(g)
    s_pts = g.uniform(-1.0, 1.0, (frames * N, 3)).astype(np.float32)
    if strided:   # queries that are not support points
        q_pts = g.uniform(-1.0, 1.0, (frames * M, 3)).astype(np.float32)
    else:
        q_pts = np.concatenate([s_pts[f * N:f * N + M] for f in range(frames)], 0)
    idx = g.integers(0, N + 1, (frames * M, H)).astype(np.int32)
    idx[::3, H // 2:] = N
    feats = g.standard_normal((frames * N, C)).astype(np.float32)
    feats[::5] = 0
    return G(feats), G(q_pts), G(s_pts), G(idx), G(kp)


# C -> kernel form: 4 c4, 20 <1,1>, 32 <2,1>, 64 <4,1>, 128 <4,2>, 256 shared<2>, 512 shared<4>
@pytest.mark.parametrize("frames", [1, 3])
@pytest.mark.parametrize("C", [4, 20, 32, 64, 128, 256, 512])
def test_records_path_equals_separate_arrays(ops, monkeypatch, C, frames):
    M, N = 8, 64
    g = np.random.default_rng(1000 * C + frames)
    for H in (4, 68, 128):
        feats, q_pts, s_pts, idx, kp = _random_case(g, frames, M, N, H, C, False)
        perm = G(np.concatenate([g.permutation(M) for _ in range(frames)]).astype(np.int32))
        for order in (None, perm):
            for planes in (False, True):
                a0, c0 = _aggregate(ops, monkeypatch, False, feats, q_pts, s_pts, idx, kp, SIGMA, frames=frames, order=order, planes=planes)
                a1, c1 = _aggregate(ops, monkeypatch, True, feats, q_pts, s_pts, idx, kp, SIGMA, frames=frames, order=order, planes=planes)
                assert a0.dtype == a1.dtype and torch.equal(a0, a1), (C, frames, H, order is not None, planes)
                assert torch.equal(c0, c1), (C, frames, H, order is not None, planes)
                assert H == 4 or float(a1.float().abs().max()) > 0   # hundreds of neighbours: some lie inside the support


@pytest.mark.parametrize("C", [32, 256])
def test_records_path_strided(ops, monkeypatch, C):
    N, frames = 64, 3
    M = N // 2
    g = np.random.default_rng(77 + C)
    feats, q_pts, s_pts, idx, kp = _random_case(g, frames, M, N, 68, C, True)
    for planes in (False, True):
        a0, c0 = _aggregate(ops, monkeypatch, False, feats, q_pts, s_pts, idx, kp, SIGMA, frames=frames, planes=planes)
        a1, c1 = _aggregate(ops, monkeypatch, True, feats, q_pts, s_pts, idx, kp, SIGMA, frames=frames, planes=planes)
        assert torch.equal(a0, a1) and torch.equal(c0, c1)


def _kpconv_fp64(feats, q_pts, s_pts, idx, kp, sigma):
    """kpconv.py:91-116 up to the weights: -> (agg (M, 15, C), number of neighbours whose feature row sums to > 0, not clamped)."""
    f = torch.cat([feats.double(), torch.zeros(1, feats.shape[1], dtype=torch.float64)], 0)
    s = torch.cat([s_pts.double(), torch.full((1, 3), 1e6, dtype=torch.float64)], 0)
    nb = s[idx.long()] - q_pts.double()[:, None]                       # (M, H, 3)
    d = (nb[:, :, None, :] - kp.double()[None, None]).pow(2).sum(-1).sqrt()   # (M, H, 15)
    w = (1.0 - d / sigma).clamp(min=0.0)
    nf = f[idx.long()]                                                 # (M, H, C)
    return torch.einsum("mhk,mhc->mkc", w, nf), (nf.sum(-1) > 0).sum(-1)


N_OUT, N_IN, H_SUP = 150, 150, 128


@pytest.fixture(scope="module")
def support_scene():
    """Support points at chosen distances from one spot: rows [0, 150) outside the support max|kp| + sigma (1.05 ... 3 radii), rows
    [150, 300) inside (0 ... 0.95 radii); row 0 holds large finite features.  Shared, never modified."""
    g = np.random.default_rng(5)
    kp = _kernel_points(g)
    rs = _rsup(kp)
    centre = np.array([0.3, -0.2, 0.1])
    dirs = g.standard_normal((N_OUT + N_IN, 3))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    # the queries sit within 0.004 of the centre: far less than the 5 % margins on either side of the support radius
    dist = np.concatenate([g.uniform(1.05, 3.0, N_OUT), g.uniform(0.0, 0.95, N_IN)]) * rs
    s_pts = (centre + dirs * dist[:, None]).astype(np.float32)
    q_pts = (centre + 0.001 * np.arange(4)[:, None]).astype(np.float32)
    return kp, s_pts, q_pts


def _support_rows(g, nin):
    """(4, 128) indices: queries 0..2 with exactly `nin` neighbours inside the support, none of them first in the row (unless all 128
    are inside), the rest outside points and shadows; query 3 always two inside, shadows and outside points."""
    idx = np.empty((4, H_SUP), dtype=np.int32)
    for m in range(4):
        n = nin if m < 3 else 2
        row = g.integers(0, N_OUT, H_SUP)                          # outside points (row 0 among them)
        row[g.random(H_SUP) < 0.3] = N_OUT + N_IN                  # shadows
        row[5], row[H_SUP - 1] = N_OUT + N_IN, 0
        slots = np.arange(H_SUP) if n == H_SUP else 1 + g.permutation(H_SUP - 1)[:n]
        row[slots] = N_OUT + g.permutation(N_IN)[:n]
        idx[m] = row
    return idx


@pytest.mark.parametrize("C", [32, 128, 256])
@pytest.mark.parametrize("nin", [0, 1, 3, 4, 5, 12, 13, 16, 17, 128])
def test_neighbour_counts_in_support(ops, monkeypatch, support_scene, nin, C):
    """Tolerance: rtol = atol = 1e-4, what test_kpconv_random (tests/test_ops_gpu.py) allows."""
    kp, s_pts, q_pts = support_scene
    g = np.random.default_rng(100 * nin + C)
    idx = _support_rows(g, nin)
    feats = g.standard_normal((N_OUT + N_IN, C)).astype(np.float32)
    feats[0] = 1e30   # the row shadow records point at: finite
    feats[N_OUT + 3] = 0
    ref, npos = _kpconv_fp64(*(torch.from_numpy(x) for x in (feats, q_pts, s_pts, idx, kp)), SIGMA)
    inside = (torch.from_numpy(idx) >= N_OUT) & (torch.from_numpy(idx) < N_OUT + N_IN)
    assert inside[:3].sum(1).tolist() == [nin] * 3 and int(inside[3].sum()) == 2
    assert (idx == N_OUT + N_IN).any() and (nin == H_SUP or not inside[:3, 0].any())
    for records in (True, False):
        agg, cnt = _aggregate(ops, monkeypatch, records, G(feats), G(q_pts), G(s_pts), G(idx), G(kp), SIGMA)
        agg = agg.cpu().reshape(4, 15, C)
        assert bool(torch.isfinite(agg).all())
        np.testing.assert_allclose(agg.numpy(), ref.float().numpy(), rtol=1e-4, atol=1e-4)
        if nin == 0:
            assert float(agg[:3].abs().max()) == 0.0
        assert float(ref[:3].abs().max()) > 0.0 or nin < 12   # a dozen neighbours inside the support: some kernel point sees one
        flags = ops.row_sum_positive(G(feats)).cpu().long()
        flags = torch.cat([flags, torch.zeros(1, dtype=torch.long)])
        want = flags[torch.from_numpy(idx).long()].sum(1).clamp(min=1).float()
        assert torch.equal(cnt.cpu(), want)
        assert torch.equal(flags[torch.from_numpy(idx).long()].sum(1), npos)   # no row of this scene sums to within rounding of zero


@pytest.mark.parametrize("C", [20, 64, 512])
def test_flags_and_cnt(ops, monkeypatch, support_scene, C):
    """Rows summing to exactly 0, to -2^-24 and to +2^-24 (one ulp of the 1.0 they cancel): cnt = max(npos, 1) with npos counted over
    every neighbour, inside the support or not; a row of queries that meets no positive row gives 1."""
    kp, s_pts, q_pts = support_scene
    N = N_OUT + N_IN
    feats = np.zeros((N, C), dtype=np.float32)
    one_m = np.nextafter(np.float32(1.0), np.float32(0.0))
    kind = np.arange(N) % 3                                     # 0: zero row, 1: negative by one ulp, 2: positive by one ulp
    feats[kind == 1, 3], feats[kind == 1, 17] = -1.0, one_m
    feats[kind == 2, 3], feats[kind == 2, 17] = 1.0, -one_m
    g = np.random.default_rng(C)
    idx = g.integers(0, N + 1, (4, H_SUP)).astype(np.int32)
    nonpos = np.flatnonzero(kind != 2)
    idx[1] = nonpos[g.integers(0, len(nonpos), H_SUP)]          # all non-positive -> cnt 1
    idx[2] = N                                                  # all shadows -> cnt 1
    idx[3, :] = np.where(np.arange(H_SUP) % 2 == 0, 2, N)       # a positive row outside the support, 64 times
    assert kind[2] == 2
    padded = np.concatenate([kind, [0]])
    want = torch.from_numpy(np.maximum((padded[idx] == 2).sum(1), 1).astype(np.float32))
    assert want[1] == 1 and want[2] == 1 and want[3] == 64
    for records in (True, False):
        _, cnt = _aggregate(ops, monkeypatch, records, G(feats), G(q_pts), G(s_pts), G(idx), G(kp), SIGMA)
        assert torch.equal(cnt.cpu(), want), records
    recs = ops.kp_pack_support(G(feats), G(s_pts)).cpu()
    assert torch.equal(recs[:, 3], torch.from_numpy((kind == 2).astype(np.float32)))
    assert torch.equal(recs[:, 3] != 0, ops.row_sum_positive(G(feats)).cpu() != 0)


# rows per frame: 128 = whole passes of every workgroup; 100 = the last pass of the row loop is partly past the end (its clamped rows
# load, take part in nothing and store nothing) - one frame, since stack mode needs whole 64-row statistics slabs per frame
@pytest.mark.parametrize("frames,rows", [(1, 128), (3, 128), (1, 100)])
@pytest.mark.parametrize("C", [32, 128, 256])
def test_apply_kernels_emit_records(ops, monkeypatch, C, frames, rows):
    """Both apply kernels (statistics as a tensor: group_norm_apply_kernel; as a GEMM's partials: group_norm_apply_fused_kernel),
    each with and without a residual: xyz words = the points bit for bit, flag = row_sum_positive of the output; and
    cofi_kp_pack_support builds the same table from the output."""
    monkeypatch.setenv("COFI_KPCONV_RECORDS", "1")
    groups = 32
    M = rows * frames
    g = torch.Generator().manual_seed(C + frames + rows)
    # GroupNorm keeps a row's offset: rows shifted up or down by three standard deviations, through weights of positive mean, give
    # output rows whose sums are clearly positive or clearly negative, about half each
    sign = (torch.rand(M, 1, generator=g) < 0.5).float() * 2 - 1
    a = (torch.randn(M, 64, generator=g) + 3 * sign).to(DEV)
    w = (torch.randn(C, 64, generator=g) / 8 + 0.05).to(DEV)
    gamma, beta = (1 + 0.1 * torch.randn(C, generator=g)).to(DEV), (0.1 * torch.randn(C, generator=g)).to(DEV)
    res = torch.randn(M, C, generator=g).to(DEV)
    pts = torch.randn(M, 3, generator=g).to(DEV)
    y, part = ops.gemm_colstats(a, w, frames=frames)
    partials = ops.ColStats(part, M, groups, frames)
    assert partials.fusable()
    tensor = ops.group_stats(y, groups, frames=frames)
    for stats in (tensor, partials):
        for r in (None, res):
            out = ops.group_norm_apply(y, stats, gamma, beta, slope=0.1, res=r, frames=frames, want_row_pos=True, points=pts)
            torch.cuda.synchronize()
            assert getattr(out, "cofi_row_pos", None) is None
            recs, ptr = out.cofi_kp_records
            assert ptr == pts.data_ptr() and recs.shape == (M, 4) and recs.data_ptr() % 16 == 0
            assert torch.equal(recs[:, :3].contiguous().view(torch.int32), pts.view(torch.int32))
            flag = ops.row_sum_positive(out)
            assert torch.equal(recs[:, 3], flag.float())
            assert M // 8 < int(flag.sum()) < M - M // 8   # rows of both kinds
            assert torch.equal(ops.kp_pack_support(out, pts).view(torch.int32), recs.view(torch.int32))
            # the same call without points: row_pos as before, the same output
            out0 = ops.group_norm_apply(y, stats, gamma, beta, slope=0.1, res=r, frames=frames, want_row_pos=True)
            assert torch.equal(out0, out) and torch.equal(out0.cofi_row_pos, flag) and getattr(out0, "cofi_kp_records", None) is None


@pytest.mark.parametrize("C,M,frames", [(32, 64, 1), (64, 48, 3)])
def test_fused_kernel_records_on_and_off(ops, monkeypatch, C, M, frames):
    """cofi_kpconv_fused_rec against cofi_kpconv_fused: output and statistics partials bit for bit (both kernel forms: 32 channels with
    128 neighbours per phase, 64 channels with 64), with a processing order, shadows and an empty row."""
    monkeypatch.setattr(ops, "GEMM_MODE", "bf16x3")
    N, H = 96, 128
    g = np.random.default_rng(C + M)
    feats, q_pts, s_pts, idx, kp = _random_case(g, frames, M, N, H, C, True)
    idx[5, :] = N
    w = ops.presplit(G((g.standard_normal((C, 15 * C)) * 0.1).astype(np.float32)))
    b = G(g.standard_normal(C).astype(np.float32))
    order = G(np.concatenate([g.permutation(M) for _ in range(frames)]).astype(np.int32))
    assert ops.kpconv_fused_slab_rows(C, M, frames) == 16
    out = []
    for records in ("1", "0"):
        monkeypatch.setenv("COFI_KPCONV_RECORDS", records)
        y, part, sr = ops.kpconv_fused(feats, q_pts, s_pts, idx, kp, SIGMA, w, b, stat_width=1, frames=frames, order=order)
        torch.cuda.synchronize()
        out.append((y, part))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    assert bool(torch.isfinite(out[0][0]).all()) and float((out[0][0] - b).abs().max()) > 0
    assert torch.equal(out[0][0][5], b)   # no neighbour: the bias


def test_run_block_records_on_and_off(monkeypatch):
    """encoder1_2 (a residual block, 64 -> 128 through 32 channels) on a 256-point cloud in the flagship arithmetic."""
    from cofii2p_amd import kpfpn, ops, spec
    from cofii2p_amd.network import CoFiI2P

    class Opt:
        img_H, img_W, img_fine_resolution_scale, norm = 160, 512, 32, "gn"

    P = CoFiI2P(Opt(), arithmetic="bf16x6").to(DEV).eval()._pack(torch.device(DEV))
    blk = [b for b in spec.ENCODER if b.name == "encoder1_2"][0]
    assert blk.kind == "res" and blk.cin != blk.mid
    kp = P["pc_encoder.%s.KPConv.kernel_points" % blk.name].cpu().numpy()
    rs = _rsup(kp) - SIGMA + blk.sigma
    g = torch.Generator().manual_seed(3)
    pts = ((torch.rand(256, 3, generator=g) * 2 - 1) * 2 * rs).to(DEV)   # about 6 % of the cloud inside a query's support
    idx = torch.cdist(pts, pts).topk(128, largest=False).indices.to(torch.int32).contiguous()
    feats = torch.randn(256, blk.cin, generator=g).to(DEV)
    outs = []
    for records in ("1", "0"):
        monkeypatch.setenv("COFI_KPCONV_RECORDS", records)
        with torch.no_grad(), ops.arithmetic("bf16x6"):
            outs.append(kpfpn.run_block(P, blk, feats, pts, pts, idx))
        torch.cuda.synchronize()
    assert bool(torch.isfinite(outs[0]).all()) and float(outs[0].abs().max()) > 0
    assert torch.equal(outs[0], outs[1])
