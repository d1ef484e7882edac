"""The match-selection kernels of csrc/matching.hip (row_argmin_1m, select_matches, extract_patches_nhwc, fine_match, match_finish)
against a few lines of plain torch / numpy on the CPU, at the sizes where their loops change behaviour.  Needs a real MI355X.

tests/test_ops_gpu.py covers them with one recorded frame (N = 1280 = 5 x 256, a 64 x 20 map, P = 1280) and compares the fused
match_finish with the five stand-alone kernels only.  Here: N that is no multiple of the 256-thread compaction chunk, several frames
that stop at different thresholds or at none, scores equal to a threshold, pixels on both sides of every border, a second map size,
P below / at / above one wave, exact ties in both arg-searches, C that is no multiple of the four channel groups, and counts below
the capacity with sentinel-filled outputs.  Every comparison is exact unless stated otherwise.

Mutation check, on an MI355X.  `pos = off` in place of `off + popcount` in select_matches' compaction fails both select_matches tests
at every N but 1; a stride of 128 in row_argmin_1m's loop fails test_row_argmin_1m at (130, 1280) and (3, 5000) and the tie test."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import cofi_oracle as O  # noqa: E402

DEV = "cuda:0"
THR = np.array(O.score_thresholds(), dtype=np.float32)   # 0.9, 0.88, ... as the kernel receives them
MAPS = {"64x20": (64, 20, 62, 18), "100x56": (100, 56, 97, 53)}   # W8, H8, x_max, y_max


@pytest.fixture(scope="module")
def ops():
    from cofii2p_amd import ops as _ops

    assert torch.cuda.is_available()
    return _ops


@pytest.fixture(scope="module")
def lib():
    from cofii2p_amd import _lib

    return _lib.load()


def gen(seed):
    return torch.Generator().manual_seed(seed)


def G(t):
    return t.to(DEV)


def P(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------------------------------ row_argmin_1m
@pytest.mark.parametrize("N,Pn", [(1, 1), (5, 63), (7, 64), (9, 65), (130, 1280), (3, 5000)])
def test_row_argmin_1m(ops, N, Pn):
    """torch.argmin(1 - sim) in float32: the same single rounding, so the same index - sim contiguous and as a column slice of a wider
    matrix (lds > P)"""
    wide = torch.randn(N, Pn + 11, generator=gen(10007 * N + Pn))
    sim = wide[:, 5:5 + Pn]
    want = torch.argmin(1.0 - sim, dim=1).int()
    gw = G(wide)
    assert torch.equal(ops.row_argmin_1m(gw[:, 5:5 + Pn]).cpu(), want)
    assert torch.equal(ops.row_argmin_1m(gw[:, 5:5 + Pn].contiguous()).cpu(), want)


def test_row_argmin_1m_ties_constant_rows_and_infinities(ops):
    """the first index wins an exact tie: between neighbouring lanes, within one lane on a later trip, and when the later index sits in
    a lower lane; a constant row gives 0; -inf entries (1 - sim = +inf) never win"""
    Pn, top = 200, 7.0
    sim = torch.randn(8, Pn, generator=gen(3)).clamp(-3, 3)
    sim[0, 10] = sim[0, 11] = top          # p and p + 1
    sim[1, 10] = sim[1, 74] = top          # p and p + 64: one lane, two trips
    sim[2, 133] = sim[2, 70] = top         # lane 6 on its second trip against lane 5 on its third
    sim[3, 199] = sim[3, 64] = sim[3, 128] = top
    sim[4, :] = 0.3                        # constant
    sim[5, ::3] = float("-inf")
    sim[5, 0] = float("-inf")
    sim[6, :] = -0.25                      # constant behind a run of -inf
    sim[6, :3] = float("-inf")
    sim[7, :] = float("-inf")              # one finite entry
    sim[7, 150] = -2.0
    want = torch.argmin(1.0 - sim, dim=1).int()
    assert want[:5].tolist() == [10, 10, 70, 64, 0] and want[6:].tolist() == [3, 150]
    assert torch.equal(ops.row_argmin_1m(G(sim)).cpu(), want)


# ----------------------------------------------------------------------------------------------------------------- select_matches
def ref_select(score, pix, W8, x_max, y_max, min_matches, thr=THR):
    """the first threshold whose survivors (score >= thr[t], pixel inside the border) number >= min_matches -> sel, xy, (n, t);
    none -> (0, -1)"""
    score, pix = np.asarray(score, dtype=np.float32), np.asarray(pix)
    x, y = pix % W8, pix // W8
    inside = (x >= 2) & (x <= x_max) & (y >= 2) & (y <= y_max)
    for t in range(len(thr)):
        ok = (score >= thr[t]) & inside
        if int(ok.sum()) >= min_matches:
            idx = np.nonzero(ok)[0]
            return idx.astype(np.int32), np.stack([x[idx], y[idx]]).astype(np.float32), (len(idx), t)
    return None, None, (0, -1)


def border_pix(N, W8, H8, x_max, y_max, g, inside_only=False):
    """random pixels of the whole map (or of its inside), the first ones on both sides of every border"""
    lo_x, hi_x, lo_y, hi_y = (2, x_max, 2, y_max) if inside_only else (0, W8 - 1, 0, H8 - 1)
    x = torch.randint(lo_x, hi_x + 1, (N,), generator=g)
    y = torch.randint(lo_y, hi_y + 1, (N,), generator=g)
    xs, ys = ([2, x_max], [2, y_max]) if inside_only else ([1, 2, x_max, x_max + 1], [1, 2, y_max, y_max + 1])
    combos = [(a, b) for a in xs for b in ys]
    where = torch.randperm(N, generator=g)[:len(combos)]   # N < 16: some of them
    for n, (a, b) in zip(where.tolist(), combos):
        x[n], y[n] = a, b
    return (y * W8 + x).int()


def check_select(ops, score, pix, W8, H8, x_max, y_max, min_matches, frames=1):
    """one launch against ref_select, frame by frame -> the reference's (n, t) per frame"""
    sel, xy, cnt = ops.select_matches(G(score.reshape(-1)), G(pix.reshape(-1)), W8, H8, THR, min_matches=min_matches, x_max=x_max, y_max=y_max,
                                      frames=frames)
    N = score.numel() // frames
    sel, xy, cnt = sel.cpu().reshape(frames, N), xy.cpu().reshape(frames, 2, N), cnt.cpu().reshape(frames, 2)
    out = []
    for f in range(frames):
        rsel, rxy, (n, t) = ref_select(score.reshape(frames, N)[f].numpy(), pix.reshape(frames, N)[f].numpy(), W8, x_max, y_max, min_matches)
        assert cnt[f].tolist() == [n, t], (f, cnt[f].tolist(), (n, t))
        if n:
            assert np.array_equal(sel[f, :n].numpy(), rsel), f
            assert np.array_equal(xy[f, :, :n].numpy(), rxy), f
        out.append((n, t))
    return out


@pytest.mark.parametrize("map_name", list(MAPS))
@pytest.mark.parametrize("N", [1, 255, 256, 257, 1000, 1280])
def test_select_matches_one_frame(ops, N, map_name):
    W8, H8, x_max, y_max = MAPS[map_name]
    g = gen(31 * N + W8)
    # (a) random scores, some of them equal to a threshold bit for bit or one ulp below it, pixels over the whole map and on both sides
    #     of every border; the last point survives, so the ragged last chunk of the compaction holds a survivor
    score = torch.rand(N, generator=g)
    for j, n in enumerate(torch.randperm(N, generator=g)[:24].tolist()):
        thr = THR[j % 12]
        score[n] = float(thr if j % 2 == 0 else np.nextafter(thr, np.float32(0)))
    pix = border_pix(N, W8, H8, x_max, y_max, g)
    score[N - 1], pix[N - 1] = 0.95, y_max * W8 + x_max
    n1, t1 = check_select(ops, score, pix, W8, H8, x_max, y_max, 1)[0]
    assert t1 == 0 and 1 <= n1 and (N < 16 or n1 < N)
    if N >= 16:
        nm, tm = check_select(ops, score, pix, W8, H8, x_max, y_max, N // 3)[0]
        assert tm > 0 and N // 3 <= nm < N
        assert check_select(ops, score, pix, W8, H8, x_max, y_max, N)[0] == (0, -1)    # points outside the border: N is never reached
    # (b) min_matches = N, every pixel inside, and the lowest score EQUAL to threshold 7: `>=` keeps it, so the search stops there
    inside = border_pix(N, W8, H8, x_max, y_max, g, inside_only=True)
    high = 0.8 + 0.2 * torch.rand(N, generator=g)
    high[int(torch.randint(0, N, (1,), generator=g))] = float(THR[7])
    assert check_select(ops, high, inside, W8, H8, x_max, y_max, N)[0] == (N, 7)
    # (c) no threshold is enough: the one point that would do lies outside
    if N == 1:
        assert check_select(ops, torch.tensor([0.95]), torch.tensor([1 * W8 + 5], dtype=torch.int32), W8, H8, x_max, y_max, 1)[0] == (0, -1)


@pytest.mark.parametrize("map_name", list(MAPS))
@pytest.mark.parametrize("N", [1, 255, 256, 257, 1000, 1280])
def test_select_matches_three_frames_stop_at_different_thresholds(ops, N, map_name):
    """one launch, three frames: satisfied at threshold 0, only at a later threshold, never (count row (0, -1))"""
    W8, H8, x_max, y_max = MAPS[map_name]
    g = gen(77 * N + W8)
    m = max(1, N // 4)
    pix = torch.stack([border_pix(N, W8, H8, x_max, y_max, g) for _ in range(3)])
    score = torch.rand(3, N, generator=g)
    first = torch.randperm(N, generator=g)[:m]
    for f in (0, 1):
        pix[f, first] = border_pix(m, W8, H8, x_max, y_max, g, inside_only=True)
    score[0, first] = 0.9 + 0.1 * torch.rand(m, generator=g)
    score[0, first[0]] = float(THR[0])                 # equal to threshold 0
    score[1] = 0.85 * score[1]                         # nothing reaches thresholds 0 ... 2
    score[1, first[0]] = float(THR[5])
    pix[2] = (pix[2] // W8) * W8 + (pix[2] % 2)        # frame 2: x in {0, 1} - outside whatever the score
    score[2] = 0.9 + 0.1 * score[2]
    got = check_select(ops, score, pix, W8, H8, x_max, y_max, m, frames=3)
    assert got[0][1] == 0 and got[0][0] >= m
    assert got[1][1] > 2 and got[1][0] >= m
    assert got[2] == (0, -1)


# ----------------------------------------------------------------------------------------------------------- extract_patches_nhwc
def ref_patches(fmap, H2, W2, xy, scale):
    """fmap (H2 * W2, C) pixel-major, xy (2, n) -> (n, C, 16): rows top .. top + 3, columns left .. left + 3, zero outside the map"""
    C = fmap.shape[1]
    pad = torch.zeros(H2 + 8, W2 + 8, C)
    pad[4:4 + H2, 4:4 + W2] = fmap.reshape(H2, W2, C)
    left, top = torch.floor(xy[0] * scale - 2.0).long(), torch.floor(xy[1] * scale - 2.0).long()
    ar = torch.arange(4)
    rows, cols = top[:, None] + ar + 4, left[:, None] + ar + 4
    return pad[rows[:, :, None], cols[:, None, :]].permute(0, 3, 1, 2).reshape(-1, C, 16)


def patch_centres(H2, W2, scale, n, g):
    """centres that include 0 and the last row and column: windows leave the map on every side"""
    nx, ny = (W2, H2) if scale == 1 else ((W2 + 1) // 4 + 1, (H2 + 1) // 4 + 1)   # scale 4: up to the last window that touches the map
    xy = torch.stack([torch.randint(0, nx, (n,), generator=g), torch.randint(0, ny, (n,), generator=g)]).float()
    corners = [(0, 0), (nx - 1, 0), (0, ny - 1), (nx - 1, ny - 1), (1, 1), (nx - 2, ny - 2)]
    for i, (a, b) in enumerate(corners):
        xy[0, i], xy[1, i] = a, b
    if scale == 1:
        xy[:, len(corners):len(corners) + 4] += 0.5   # val-style centres between pixels: floor() decides
    return xy


SENTINEL = -777.25


@pytest.mark.parametrize("scale", [1, 4])
@pytest.mark.parametrize("C", [1, 12, 64, 128])
def test_extract_patches_nhwc(lib, C, scale):
    """torch indexing with zero padding; the map as a column slice of a wider one (ldf > C); count < capacity leaves the rows at and
    beyond the count untouched"""
    H2, W2, n, cap = 11, 17, 21, 26
    g = gen(100 * C + scale)
    wide = torch.randn(H2 * W2, C + 3, generator=g)
    fmap = wide[:, 2:2 + C]
    xy = torch.zeros(2, cap)
    xy[:, :n] = patch_centres(H2, W2, scale, n, g)
    xy[:, n:] = 1.0
    want = ref_patches(fmap, H2, W2, xy[:, :n], float(scale))
    assert bool((want[0] == 0).any()) and bool((want[3] == 0).any()) and bool((want != 0).any())   # windows do leave the map
    gw, gxy = G(wide), G(xy)
    for count in (n, cap + 3):   # the count is clamped to the capacity
        out = torch.full((cap, C, 16), SENTINEL, device=DEV)
        cnt = torch.tensor([count, 0], dtype=torch.int32, device=DEV)
        rc = lib.cofi_extract_patches_nhwc(P(gw[:, 2:2 + C]), gw.stride(0), C, H2, W2, P(gxy), gxy.stride(0), float(scale), P(cnt), cap, P(out),
                                           _stream())
        assert rc == 0
        m = min(count, cap)
        assert torch.equal(out[:m].cpu(), ref_patches(fmap, H2, W2, xy[:, :m], float(scale)))
        assert bool((out[m:] == SENTINEL).all())


# --------------------------------------------------------------------------------------------------------------------- fine_match
def cos64(patches, pc):
    """float64 cosine similarity, eps 1e-8 per norm: (n, C, 16), (n, C) -> (n, 16)"""
    p, f = patches.double(), pc.double()
    dot = (p * f[:, :, None]).sum(1)
    return dot / (p.norm(dim=1).clamp_min(1e-8) * f.norm(dim=1).clamp_min(1e-8)[:, None])


def run_fine_match(lib, patches, pc, xy, count, scale):
    """through the C ABI on sentinel-filled outputs; pc may be a column slice -> fine_xy (2, cap), best (cap,) on the CPU"""
    cap, C, _ = patches.shape
    fine_xy = torch.full((2, cap), SENTINEL, device=DEV)
    best = torch.full((cap,), -5, dtype=torch.int32, device=DEV)
    cnt = torch.tensor([count, 0], dtype=torch.int32, device=DEV)
    rc = lib.cofi_fine_match(P(patches), P(pc), pc.stride(0), C, P(xy), xy.stride(0), float(scale), P(cnt), cap, P(fine_xy), P(best), _stream())
    assert rc == 0
    return fine_xy.cpu(), best.cpu()


def want_fine_xy(xy, best, scale):
    """xy * scale - 2 + (best // 4, best % 4) in float32, the reference's x / y swap kept (x receives the quotient)"""
    b = best.long()
    base = xy * np.float32(scale) - np.float32(2.0)
    return torch.stack([base[0] + (b // 4).float(), base[1] + (b % 4).float()])


@pytest.mark.parametrize("C", [1, 13, 64, 128])
def test_fine_match_random(lib, C):
    """the pick's float64 similarity is within 1e-6 of the float64 row maximum (any correct float32 evaluation is; a wrong lane or
    channel split is not), fine_xy is exact, rows at and beyond the count keep their sentinel"""
    cap, n = 40, 33
    g = gen(500 + C)
    patches = torch.randn(cap, C, 16, generator=g) * 10.0 ** (2 * torch.rand(cap, 1, 16, generator=g) - 1)
    wide = torch.randn(cap, C + 5, generator=g)
    pc = wide[:, 1:1 + C]
    xy = torch.stack([torch.randint(0, 64, (cap,), generator=g), torch.randint(0, 20, (cap,), generator=g)]).float()
    gw = G(wide)
    fine_xy, best = run_fine_match(lib, G(patches), gw[:, 1:1 + C], G(xy), n, 4.0)
    assert bool(((best[:n] >= 0) & (best[:n] < 16)).all())
    sim = cos64(patches, pc)[:n]
    picked = sim.gather(1, best[:n].long()[:, None])[:, 0]
    assert float((sim.max(1).values - picked).max()) <= 1e-6
    assert len(set(best[:n].tolist())) > (1 if C == 1 else 8)   # the picks do spread over the pixels
    assert torch.equal(fine_xy[:, :n], want_fine_xy(xy[:, :n], best[:n], 4.0))
    assert bool((best[n:] == -5).all()) and bool((fine_xy[:, n:] == SENTINEL).all())


def test_fine_match_one_channel_is_all_ties(lib):
    """C = 1: the cosine of two scalars is +-1 - exactly so in float32 too, since sqrt(fl(x^2)) = |x| and the numerator and the
    denominator round the same product - so every row is a tie between its pixels of the descriptor's sign: the lowest of them wins,
    and index 0 where there is none (all similarities are -1)"""
    cap = 12
    g = gen(899)
    patches, pc = torch.randn(cap, 1, 16, generator=g), torch.randn(cap, 1, generator=g)
    patches[0, 0, :] = -patches[0, 0, :].abs() * torch.sign(pc[0, 0])   # no pixel of the descriptor's sign
    patches[1, 0, :15] = -patches[1, 0, :15].abs() * torch.sign(pc[1, 0])
    patches[1, 0, 15] = pc[1, 0]                                        # only the last one
    sim = cos64(patches, pc)
    assert bool((sim.abs() == 1.0).all())
    want = [int(torch.argmax((sim[i] == sim[i].max()).int())) for i in range(cap)]
    assert want[:2] == [0, 15] and len(set(want)) > 2
    xy = torch.stack([torch.arange(cap), torch.arange(cap) + 2]).float()
    fine_xy, best = run_fine_match(lib, G(patches), G(pc), G(xy), cap, 4.0)
    assert best.tolist() == want
    assert torch.equal(fine_xy, want_fine_xy(xy, best, 4.0))


@pytest.mark.parametrize("C", [13, 64, 128])
def test_fine_match_ties_and_zero_descriptor(lib, C):
    """the best patch pixel copied to a second position: the lower index wins; a zero descriptor (and a zero patch): all similarities
    are 0, index 0"""
    pairs = [(3, 12), (0, 15), (7, 8), (5, 6), (2, 14), (9, 10)]   # across and within the butterfly's halves
    cap = len(pairs) + 2
    g = gen(900 + C)
    patches, pc = torch.randn(cap, C, 16, generator=g), torch.randn(cap, C, generator=g)
    for i, (lo, hi) in enumerate(pairs):
        patches[i, :, hi] = patches[i, :, lo] = 1.5 * pc[i] + 0.05 * torch.randn(C, generator=g)
    pc[cap - 2] = 0.0
    pc[cap - 1] = 0.0
    patches[cap - 1] = 0.0
    sim = cos64(patches, pc)
    for i, (lo, hi) in enumerate(pairs):
        assert sim[i, lo] == sim[i, hi] == sim[i].max() and int((sim[i] == sim[i].max()).sum()) == 2
    xy = torch.stack([torch.arange(cap), torch.arange(cap) + 2]).float()
    fine_xy, best = run_fine_match(lib, G(patches), G(pc), G(xy), cap, 4.0)
    assert best.tolist() == [lo for lo, _ in pairs] + [0, 0]
    assert torch.equal(fine_xy, want_fine_xy(xy, best, 4.0))


# ------------------------------------------------------------------------------------------------------------------- match_finish
def _finish_inputs(C, frames, cap, N4, N1, H2, W2, g):
    pts1 = torch.randn(frames * N1, 3, generator=g)
    pts4 = torch.randn(frames * N4, 3, generator=g)
    fmap, fpc = torch.randn(frames * H2 * W2, C, generator=g), torch.randn(frames * N1, C, generator=g)
    sel = torch.stack([torch.sort(torch.randperm(N4, generator=g)[:cap]).values for _ in range(frames)]).int()
    xy = torch.stack([torch.stack([torch.randint(0, (W2 + 1) // 4 + 1, (cap,), generator=g), torch.randint(0, (H2 + 1) // 4 + 1, (cap,), generator=g)])
                      for _ in range(frames)]).float()
    return pts4, pts1, sel, fmap, xy, fpc


def test_match_finish_three_frames_equal_three_calls(ops):
    """frames = 3 with counts (cap, 5, 0): every output's first `count` rows equal the single-frame call on that frame's blocks bit for
    bit; cap != N4, so a frame offset taken from the wrong size shows"""
    C, frames, cap, N4, N1, H2, W2 = 13, 3, 24, 40, 300, 11, 17
    pts4, pts1, sel, fmap, xy, fpc = _finish_inputs(C, frames, cap, N4, N1, H2, W2, gen(41))
    counts = [cap, 5, 0]
    cnt = torch.tensor([[counts[0], 0], [counts[1], 2], [counts[2], -1]], dtype=torch.int32)
    outs = ops.match_finish(G(pts4), G(pts1), G(sel), G(cnt), G(fmap), H2, W2, G(xy), G(fpc), 4.0, frames=frames)
    assert outs[0].shape == (frames, cap, 3) and outs[1].shape == (frames, cap, C, 16) and outs[3].shape == (frames, 2, cap)
    for f, n in enumerate(counts):
        blk = lambda t, rows: G(t[f * rows:(f + 1) * rows].contiguous())
        one = ops.match_finish(blk(pts4, N4), blk(pts1, N1), G(sel[f].contiguous()), G(cnt[f].contiguous()), blk(fmap, H2 * W2), H2, W2,
                               G(xy[f].contiguous()), blk(fpc, N1), 4.0)
        for k, (a, b) in enumerate(zip(outs, one)):
            a, b = (a[f][:, :n], b[:, :n]) if k == 3 else (a[f][:n], b[:n])
            assert a.shape == b.shape and torch.equal(a, b), (f, k)
        if n:   # and the single-frame call is what plain indexing gives
            assert torch.equal(one[0][:n].cpu(), pts4[f * N4:(f + 1) * N4][sel[f, :n].long()])
            assert torch.equal(one[1][:n].cpu(), ref_patches(fmap[f * H2 * W2:(f + 1) * H2 * W2], H2, W2, xy[f][:, :n], 4.0))
            d = ((pts4[f * N4:(f + 1) * N4][sel[f, :n].long()][:, None, :].double() - pts1[f * N1:(f + 1) * N1][None].double()) ** 2).sum(-1)
            assert torch.equal(one[2][:n].cpu(), fpc[f * N1:(f + 1) * N1][d.argmin(1)])   # random points: no near-ties in the node search
            assert torch.equal(one[3][:, :n].cpu(), want_fine_xy(xy[f][:, :n], one[4][:n].cpu(), 4.0))


def test_match_finish_rejects_more_than_128_channels(ops):
    from cofii2p_amd import _lib

    C, cap, N4, N1, H2, W2 = 129, 4, 6, 10, 5, 6
    pts4, pts1, sel, fmap, xy, fpc = _finish_inputs(C, 1, cap, N4, N1, H2, W2, gen(43))
    cnt = torch.tensor([cap, 0], dtype=torch.int32)
    with pytest.raises(_lib.CofiError, match="COFI_EUNSUPPORTED"):
        ops.match_finish(G(pts4), G(pts1), G(sel[0].contiguous()), G(cnt), G(fmap), H2, W2, G(xy[0].contiguous()), G(fpc), 4.0)
    torch.cuda.synchronize()
