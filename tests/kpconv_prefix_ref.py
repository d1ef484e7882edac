"""numpy-float32 emulation of what the SORTED KPConv aggregation kernels (csrc/kpconv.hip) decide per neighbour row: the canonical KNN
distance the rows are sorted by (csrc/knn_common.h), the kernel's support test, the stop rule of the chunked record gather
(kp_prefix_done) and the flag bit table (kp_pack_bits_kernel).  Shared by tests/test_kpconv_prefix_cpu.py, tests/test_kpconv_prefix_gpu.py
and tools/kpconv_probe.py; needs neither a GPU nor the built library."""
import numpy as np

F = np.float32
CHUNK_ENDS = (16, 64, 128)   # the record gather covers neighbours [0, 16), then [16, 64), then [64, 128)


def _fma(a, b, c):
    """fp32 fused multiply-add: the product of two fp32 is exact in fp64, the sum is rounded to fp64 and then to fp32"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)


def sqnorm(p):
    """canon_sqnorm: (x x + y y) + z z, every operation rounded to fp32"""
    p = p.astype(F)
    return (p[..., 0] * p[..., 0] + p[..., 1] * p[..., 1]) + p[..., 2] * p[..., 2]


def canon_dist(q, s):
    """canon_dist of knn_common.h for queries q (R, 3) and neighbours s (R, H, 3) -> (R, H) fp32"""
    q, s = q.astype(F)[:, None, :], s.astype(F)
    dot = _fma(q[..., 2], s[..., 2], _fma(q[..., 1], s[..., 1], q[..., 0] * s[..., 0]))
    d = ((F(-2.0) * dot) + sqnorm(q)) + sqnorm(s)
    return np.maximum(d, F(1e-12))


def kernel_d2(q, s):
    """the squared distance the aggregation kernels test against the support: differences first, then (dx dx + dy dy) + dz dz"""
    return sqnorm(s.astype(F) - q.astype(F)[:, None, :])


def support_radius2(kp, sigma):
    """kp_query: rsup = (max |kp| + sigma) * 1.00002, squared - all in fp32"""
    kn = np.sqrt(sqnorm(kp)).astype(F).max()
    rsup = F(F(kn + F(sigma)) * F(1.00002))
    return F(rsup * rsup)


def prefix_done(d2_last, q, rsup2):
    """kp_prefix_done: may the gather stop behind a valid neighbour at squared distance d2_last (R,) of queries q (R, 3)?"""
    qn2 = F(2.0) * np.sqrt(sqnorm(q)).astype(F)
    rsup = np.sqrt(F(rsup2)).astype(F)
    s = (qn2 + F(2.0) * np.sqrt(d2_last.astype(F)).astype(F)) + rsup
    return d2_last.astype(F) >= F(rsup2) * F(1.0 + 2.0 ** -10) + F(2.0 ** -20) * (s * s)


def sort_rows(q, s, idx):
    """every row into ascending (canonical distance, index) order, as the KNN kernels emit it -> s, idx"""
    key = canon_dist(q, s)
    o = np.lexsort((idx, key), axis=1)
    return np.take_along_axis(s, o[..., None], 1), np.take_along_axis(idx, o, 1)


def gathered(q, s, nvalid, rsup2):
    """-> (R,) how many leading neighbours of each row the chunked gather reads: s (R, H, 3) sorted rows whose first nvalid (R,) entries
    are valid indices (shadow entries behind them).  After the chunk that ends at neighbour e - 1 the wave stops if that neighbour is no
    valid index (nothing valid stands behind it) or if prefix_done holds for it."""
    R, H = s.shape[:2]
    d2 = kernel_d2(q, s)
    out = np.full(R, H, dtype=np.int64)
    open_ = np.ones(R, dtype=bool)
    for e in CHUNK_ENDS:
        if e > H:   # the chunk's last lane lies past the row: no valid index
            out[open_] = np.minimum(out[open_], H)
            open_[:] = False
            break
        stop = open_ & ((nvalid < e) | prefix_done(d2[:, e - 1], q, rsup2))
        out[stop] = e
        open_ &= ~stop
    return out


def survivors(q, s, nvalid, rsup2):
    """(R, H) bool: the neighbours the unsorted kernels keep"""
    H = s.shape[1]
    return (np.arange(H)[None, :] < nvalid[:, None]) & (kernel_d2(q, s) < F(rsup2))


def chunks(q, s, nvalid, rsup2):
    """-> (R,) 1, 2 or 3: the chunks each row's gather reads"""
    g = gathered(q, s, nvalid, rsup2)
    return 1 + (g > CHUNK_ENDS[0]).astype(np.int64) + (g > CHUNK_ENDS[1]).astype(np.int64)


def pack_bits(row_pos):
    """row_pos (frames, N) of 0 / 1 -> (frames, ceil(N / 32)) uint32 words: bit n & 31 of word n >> 5 = row_pos[n], padding bits 0"""
    row_pos = np.asarray(row_pos)
    frames, N = row_pos.shape
    bw = (N + 31) // 32
    padded = np.zeros((frames, bw * 32), dtype=np.uint64)
    padded[:, :N] = row_pos != 0
    return (padded.reshape(frames, bw, 32) << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)


def pack_bits_as_launched(row_pos):
    """the same table the way kp_pack_bits_kernel forms it: workgroups of 256 rows, a wave's 64-lane ballot, lanes 0 and 32 store one word
    each if it lies inside the frame's bw words"""
    row_pos = np.asarray(row_pos)
    frames, N = row_pos.shape
    bw = (N + 31) // 32
    out = np.zeros((frames, bw), dtype=np.uint32)
    written = np.zeros((frames, bw), dtype=np.int64)
    for f in range(frames):
        for block in range((N + 255) // 256):
            for wave in range(4):
                n0 = block * 256 + wave * 64
                ballot = 0
                for lane in range(64):
                    if n0 + lane < N and row_pos[f, n0 + lane] != 0:
                        ballot |= 1 << lane
                for lane in (0, 32):
                    w = (n0 + lane) >> 5
                    if w < bw:
                        out[f, w] = (ballot >> lane) & 0xFFFFFFFF
                        written[f, w] += 1
    assert (written == 1).all()   # every word of the table is stored exactly once
    return out
