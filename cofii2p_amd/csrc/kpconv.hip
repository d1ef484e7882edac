// KPConv part 1 (kernel-point influence + neighbour aggregation), neighbour max-pool and
// nearest up-sample gathers.  Reference: model/kpconv/kpconv.py:91-116, functional.py:5-21,53-66.
//
// kpconv_aggregate: ONE WAVE PER QUERY POINT.  The aggregation of one query,
//     agg[k, c] = sum_h w[h,k] * f[idx[h], c]      (15 x H) . (H x C),
// is an MFMA chain of v_mfma_f32_16x16x4_f32: rows = kernel points (15 padded to 16),
// cols = 16 channels, contraction over 4 neighbours per step.  Lane (g = l>>4, j = l&15) owns
// neighbour h = 4s+g in step s and
//   - computes the influence weight of kernel point k = j for that neighbour (A operand), and
//   - loads channel c0+j of that neighbour's feature row (B operand): 16 lanes read 64 contiguous
//     bytes of one row, so the gather is served in coalesced 64-B segments from L2.
// Nothing is staged through LDS and the (M,H,15) influence tensor / (M,H,C) gather of the reference
// never exist in memory.  Channel passes of 16*NACC channels go over gridDim.y.
//
// The four aggregation kernels (kpconv_aggregate_kernel, _shared_kernel, _c4_kernel, kpconv_fused_kernel) promise identical bits; they keep
// the promise by running the SAME bodies, each defined once:
//   kp_query          query position, this lane's kernel point, 1 / sigma, the support radius     (all four)
//   kp_shift_frame    stack mode: support bases of the query's frame                              (general, shared, fused)
//   kp_support        one support row's position and flag, from a record or from separate arrays  (general, shared, fused)
//   kp_compact / kp_shadow   survivors into LDS records in neighbour order, shadow records behind  (general, shared, fused; c4 fills two arrays)
//   kp_steps          the pipelined feature-load / MFMA loop over the records                     (general, shared, fused)
//   kp_store          = kp_store_rows (fp32 or bf16 planes, via kp_split_store) + kp_store_cnt    (general, shared; c4 the count; fused
//                       kp_split_store into its LDS tile and kp_count)
// (general, fused: through kp_aggregate_query).  Host side: kp_args names every KpArgs field once, kp_check_support is the addressing limit.
#include "bf16_split.h"
#include "common.h"
#include <stdlib.h>

namespace {

// XCD-aware, bijective remap of a 1-D block id: the dispatcher sends block b to XCD b % 8; remapping gives every XCD one
// CONTIGUOUS eighth of the (spatially sorted) queries, so its private 4 MB L2 only ever sees the source rows of one
// spatial region (N*C*4/8 bytes <= 1.3 MB) instead of the whole 10.5 MB source.
__device__ __forceinline__ int xcd_contiguous_block(int b, int nblk) {
    const int q = nblk >> 3, r = nblk & 7, x = b & 7, i = b >> 3;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + i;
}

struct KpArgs {
    const float *feats, *q_pts, *s_pts, *kp;
    const int32_t *idx;
    const uint8_t *row_pos;
    float *agg, *cnt;
    int ldf, N, C, M, H, ld_agg;   // N = support rows PER FRAME, M = total query rows
    float sigma;
    int Mpf;                       // query rows per frame (stack mode: frame f owns queries [f*Mpf, ..) and support [f*N, ..))
    size_t planes_lo;              // 0: agg is fp32 (M, ld_agg); else agg is a bf16 hi plane (M, ld_agg bf16) and the lo plane starts planes_lo
                                   // elements later - the GEMM that consumes it then needs no conversion (COFI_GEMM_A_SPLIT)
    const int32_t *order;          // optional processing order (frame-local query ids, stacked per frame): wave w of the grid
                                   // handles query order[w].  A spatially sorted order makes the waves resident on one CU work on
                                   // neighbouring queries whose neighbour rows overlap, so the gather is served from L1 instead of L2.
    const float4 *recs;            // REC kernels: one 16-byte record (x, y, z, flag) per support row in place of s_pts / row_pos, flag = 1.0f
                                   // where the row's feature sum is > 0 (what row_pos holds)
    // SORTED kernels (they stage from records, so row_pos is free): row_pos carries the flags as a BIT table, kp_bits() - this struct
    // keeps its layout, and with it every unsorted kernel the instruction stream it had (a longer kernarg block reschedules them)
};

// ---- SORTED forms: record gathers for the sorted prefix of a neighbour row only ---------------------------------------------------
// PROMISE of the caller (pyramid key "sorted_tables"): in every row of idx the entries inside [0, N) come first, in
// ascending order of the canonical fp32 distance of knn_common.h (canon_dist); entries outside [0, N) stand only behind them.
// The support test d2 < rsup2 is monotone in the distance, so the survivors stand at the front of the row, and the staging - one gather of a
// 16-byte record per neighbour, 64 lanes on 64 cache lines - is needed for that prefix only.  What the other neighbours contribute is
// their positive-sum flag (npos counts over ALL H neighbours); it comes from the bit table, 2.5 KB per 20 480-row frame, which stays in
// the vector L1.  The records are gathered in chunks - neighbours 0 - 15, then 16 - 63, then 64 - 127 - and the wave stops after a chunk
// as soon as nothing behind it can pass the support test.  Everything else (differences, support test, compaction, steps) is the
// unsorted form's, on the same records in the same order: identical bits on every table that keeps the promise.
//
// STOP RULE.  u = 2^-24.  For a neighbour s of query q let D = |s - q|^2 (exact), c = canon_dist (what the row is sorted by) and
// d2 = (dx dx + dy dy) + dz dz as this file computes it (what the support test reads).
//   (a) c = ((-2 dot) + qq) + ss: dot, qq, ss are three-term sums (<= 3u relative to |q||s|, |q|^2, |s|^2, fused or not), the two
//       additions round once each (u (2|q||s| + |q|^2) and u (|q| + |s|)^2):  |c - D| <= u (4|q|^2 + 4|s|^2 + 10|q||s|) (1 + O(u))
//       <= 5u (|q| + |s|)^2 =: E(s).  canon_dist's clamp at 1e-12 moves c by at most 1e-12.
//   (b) d2 = D (1 + e), |e| <= 6u < 2^-21 (one rounding per difference, relative; three products, two sums).
// Let L be the last neighbour of a chunk, valid, and X any valid neighbour behind it that passes the test: d2_X < rsup2, so
// D_X < rsup2 (1 + 2^-21) and |s_X| <= |q| + 1.01 rsup.  The row is sorted: c_X >= c_L, hence
//   D_L <= D_X + E(X) + E(L) + 1e-12,   E(X) <= 5u (2|q| + 1.01 rsup)^2,   E(L) <= 5u (2|q| + sqrt(D_L))^2,
// and with S = 2|q| + 2 sqrt(d2_L) + rsup (>= both brackets / 1.01):  d2_L (1 - 2^-21) <= D_L < rsup2 (1 + 2^-21) + 10.3u S^2 + 1e-12.
// The kernel stops after L only if   d2_L >= rsup2 (1 + 2^-10) + 2^-20 S^2   (kp_prefix_done): 16u S^2 against the 10.3u S^2 that can
// occur, and 2^-10 rsup2 against 2^-20 rsup2 + 1e-12 (rsup > 1e-4) and the roundings of evaluating the rule itself in fp32.  So no
// such X exists.  The rule reads q, rsup and L only; far from the origin it merely costs another chunk.  The other way to stop is that
// the chunk's last entry is not a valid index: by the promise nothing valid stands behind it.
// tests/kpconv_prefix_ref.py emulates (a), (b) and the rule in numpy float32; tests/test_kpconv_prefix_cpu.py holds it to zero misses.
struct KpStop {
    float qn2, rsup, rsup2;   // 2 |q|, the support radius and its square
};

__device__ __forceinline__ bool kp_prefix_done(const float d2_last, const KpStop &k) {
    const float s = k.qn2 + 2.0f * __builtin_amdgcn_sqrtf(d2_last) + k.rsup;
    return d2_last >= k.rsup2 * (1.0f + 0x1p-10f) + 0x1p-20f * (s * s);
}

// a wave-uniform value into a scalar register (it then costs no vector register across the step loop)
__device__ __forceinline__ float kp_scalar(const float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }

// SORTED: the flag bits of the frame of query m: one bit per support row (bit n & 31 of word n >> 5), (N + 31) / 32 words per frame
__device__ __forceinline__ const uint32_t *kp_bits(const KpArgs &a, const int m) {
    return reinterpret_cast<const uint32_t *>(a.row_pos) + (size_t)(m / a.Mpf) * ((a.N + 31) >> 5);
}

// value of lane `src` (compile-time) in a scalar register
__device__ __forceinline__ float kp_lane_value(const float v, const int src) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src)); }

// one flag bit per support row from the records of `frames` frames of N rows (stride floats per record, flag at float `off`):
// thread = row, a wave's ballot = two words; bw words per frame
__global__ __launch_bounds__(256) void kp_pack_bits_kernel(const float *recs, int stride, int off, int N, int bw, uint32_t *bits) {
    const int n = blockIdx.x * 256 + threadIdx.x, f = blockIdx.y;
    const bool flag = n < N && recs[((size_t)f * N + n) * stride + off] != 0.f;
    const unsigned long long m = __ballot(flag);
    const int w = n >> 5, lane = threadIdx.x & 63;
    if ((lane & 31) == 0 && w < bw) bits[(size_t)f * bw + w] = (uint32_t)(m >> lane);
}

// VEC = contiguous channels one lane loads per neighbour (1, 2 or 4 -> dword / dwordx2 / dwordx4), NCH =
// channel chunks of 16*VEC per pass.  MFMA column j of accumulator (ch, a) is channel
// c0 + ch*16*VEC + VEC*j + a: a permutation of the channel axis that turns the B-operand gather into
// 16 lanes x 4*VEC contiguous bytes per neighbour row.
//
// The texture-address unit of a CU is shared by its 4 SIMDs and spends ~16 cycles per wave-wide memory instruction,
// while one 4-neighbour step is only NCH*VEC MFMAs (32 cycles each) per SIMD: the kernel is kept to ONE feature load
// per (step, channel chunk).  Everything else a step needs - the neighbour's offset from the query, its validity, its
// row id - is staged per 64 neighbours with coalesced/gather loads by lane = neighbour, parked in a wave-private LDS
// record, and fetched back per step with one broadcast ds_read_b128 (4 distinct addresses per wave).
constexpr int KP_PHASE_DEFAULT = 128;  // neighbour records staged per wave and phase (H <= 128: one phase)
constexpr int KP_PAD = 64;     // shadow records behind the (compacted) records of a phase: the round-up to 16 neighbours (<= 15) and the
                               // pipeline's look-ahead (<= 7 steps = 28) read them

template <int VEC, int NCH>
struct KpFeat {
    float f[NCH][VEC];
};

// The MFMA / feature-load loop of one wave over the `nin` staged neighbour records of a query (rec: LDS, followed by >= 64 shadow
// records), channels coffb[] of the rows behind fbase: acc += W^T F.
template <int VEC, int NCH>
__device__ __forceinline__ void kp_steps(const char *fbase, const unsigned ldfb, const unsigned (&coffb)[NCH], const float4 *rec, const int nin,
                                         const float kx, const float ky, const float kz, const float inv_sigma, f32x4 (&acc)[NCH][VEC]) {
    const int g = (threadIdx.x & 63) >> 4;
    {
        const int steps = (nin + 3) >> 2;
        const float4 *rg = rec + g;  // record of neighbour 4t+g = rg[4t]; reads past the phase hit later records or the pad
        // The loads ARE the software pipeline.  Each one is followed by a compiler-level memory barrier (no instruction):
        // without it the optimiser folds the loop-carried loaded values into loop-carried ADDRESSES and re-issues every
        // load at its use, which serialises the L2 latency into each step.
        auto fetch = [&](int t) -> float4 {
            const float4 v = rg[4 * t];
            asm volatile("" ::: "memory");
            return v;
        };
        auto issue = [&](const float4 &rc, KpFeat<VEC, NCH> &f) {
            const unsigned id = (unsigned)__float_as_int(rc.w);
#pragma unroll
            for (int ch = 0; ch < NCH; ++ch) {
                // byte offset of (row, channel chunk): < 4 GiB with id, ldfb < 2^24 (checked by the host) -> one full-rate mad
                const char *src = fbase + (size_t)(__umul24(id, ldfb) + coffb[ch]);
                if constexpr (VEC == 4) {
                    const f32x4 tt = *reinterpret_cast<const f32x4 *>(src);
                    f.f[ch][0] = tt[0]; f.f[ch][1] = tt[1]; f.f[ch][2] = tt[2]; f.f[ch][3] = tt[3];
                } else if constexpr (VEC == 2) {
                    const f32x2 tt = *reinterpret_cast<const f32x2 *>(src);
                    f.f[ch][0] = tt[0]; f.f[ch][1] = tt[1];
                } else {
                    f.f[ch][0] = *reinterpret_cast<const float *>(src);
                }
            }
            asm volatile("" ::: "memory");
        };
        auto consume = [&](const float4 &rc, const KpFeat<VEC, NCH> &f) {
            // kpconv.py:93-99: ((s - q) - kp)^2 summed, sqrt, 1 - d/sigma, clamp at 0 (straight-line: select, no branch)
            const float dx = rc.x - kx, dy = rc.y - ky, dz = rc.z - kz;
            const float sq = (dx * dx + dy * dy) + dz * dz;
            const float w = fmaxf(1.0f - __builtin_amdgcn_sqrtf(sq) * inv_sigma, 0.0f);
#pragma unroll
            for (int ch = 0; ch < NCH; ++ch)
#pragma unroll
                for (int v = 0; v < VEC; ++v)
                    acc[ch][v] = __builtin_amdgcn_mfma_f32_16x16x4f32(w, f.f[ch][v], acc[ch][v], 0, 0, 0);
        };
        // software pipeline: slot k fetches the record of step k+3 (LDS), runs the MFMAs of step k behind it, then issues
        // the feature loads of step k+3 (L2) - three feature loads stay in flight per wave.  Exactly `steps` steps run (the
        // support holds 2 - 5 neighbours at the stages with the most queries: one or two steps): a feature load is issued only for
        // a step that exists, and the rotation is left after the last one.  All tests are wave-uniform (scalar branches); the record
        // fetches past the last step read shadow records.
        float4 R0 = fetch(0), R1 = fetch(1), R2 = fetch(2), R3;
        KpFeat<VEC, NCH> F0, F1, F2, F3;
        if (steps > 0) issue(R0, F0);
        if (steps > 1) issue(R1, F1);
        if (steps > 2) issue(R2, F2);
        int t = 0;
        for (; t + 4 <= steps; t += 4) {   // whole rounds of the rotation
            R3 = fetch(t + 3); consume(R0, F0); issue(R3, F3);
            R0 = fetch(t + 4); consume(R1, F1); if (t + 4 < steps) issue(R0, F0);
            R1 = fetch(t + 5); consume(R2, F2); if (t + 5 < steps) issue(R1, F1);
            R2 = fetch(t + 6); consume(R3, F3); if (t + 6 < steps) issue(R2, F2);
        }
        if (t < steps) {   // the last 1 - 3 steps: their loads are in flight, the rotation stands at set 0
            consume(R0, F0);
            if (t + 1 < steps) {
                consume(R1, F1);
                if (t + 2 < steps) consume(R2, F2);
            }
        }
    }
}

// What a wave knows of its query m before it looks at a neighbour: the query's position, kernel point j of this lane, 1 / sigma and the
// squared support radius.
struct KpQuery {
    float qx, qy, qz, kx, ky, kz, inv_sigma, rsup2;
};

__device__ __forceinline__ KpQuery kp_query(const KpArgs &a, const int m, const int j) {
    KpQuery q;
    q.qx = a.q_pts[3 * m]; q.qy = a.q_pts[3 * m + 1]; q.qz = a.q_pts[3 * m + 2];
    // MFMA row 15 (lane j == 15) is a padding row that is never stored: it may hold any finite weight
    const int jk = j < 15 ? j : 0;
    q.kx = a.kp[3 * jk]; q.ky = a.kp[3 * jk + 1]; q.kz = a.kp[3 * jk + 2];
    q.inv_sigma = 1.0f / a.sigma;
    // Support of the kernel: the influence max(0, 1 - |d - k| / sigma) of EVERY kernel point k is exactly 0 for a neighbour at |d| >=
    // max|k| + sigma.  The k nearest neighbours of the pyramid reach far beyond that (KITTI-shaped frames: 2 - 26 % of the 128 lie
    // inside), so the staging keeps only the neighbours inside the support (compacted, order preserved) and the MFMA / feature-load
    // loop runs over those: exact - the dropped terms are zeros - up to the regrouping of the fp32 sums.  (The bound carries a 2e-5
    // margin: far more than the rounding of the distances on either side.)
    float kn = j < 15 ? __builtin_amdgcn_sqrtf((q.kx * q.kx + q.ky * q.ky) + q.kz * q.kz) : 0.f;
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) kn = fmaxf(kn, __shfl_xor(kn, o, 64));
    const float rsup = (kn + a.sigma) * 1.00002f;
    q.rsup2 = rsup * rsup;
    return q;
}

// what kp_prefix_done reads of a query, in scalar registers
__device__ __forceinline__ KpStop kp_stop(const KpQuery &q) {
    return {kp_scalar(2.0f * __builtin_amdgcn_sqrtf((q.qx * q.qx + q.qy * q.qy) + q.qz * q.qz)), kp_scalar(__builtin_amdgcn_sqrtf(q.rsup2)), q.rsup2};
}

// Stack mode: shift the support-side bases of a (a kernel's private copy) to the frame of query m (indices are frame-local).
// REC: the support is a.recs, else a.s_pts / a.row_pos.
template <bool REC>
__device__ __forceinline__ void kp_shift_frame(KpArgs &a, const int m) {
    const size_t fo = (size_t)(m / a.Mpf) * a.N;
    a.feats += fo * a.ldf;
    if constexpr (REC) {
        a.recs += fo;
    } else {
        a.s_pts += fo * 3;
        a.row_pos += fo;
    }
}

// Position and positive-sum flag of support row idc: ONE 16-byte record (REC) or three position dwords and the flag byte.
template <bool REC>
__device__ __forceinline__ void kp_support(const KpArgs &a, const int idc, float &px, float &py, float &pz, int &pos) {
    if constexpr (REC) {
        const float4 rv = a.recs[idc];
        px = rv.x; py = rv.y; pz = rv.z;
        pos = rv.w != 0.f;
    } else {
        const float *sp = a.s_pts + 3 * (size_t)idc;
        px = sp[0]; py = sp[1]; pz = sp[2];
        pos = a.row_pos[idc];
    }
}

// Compaction: the lanes with `inside` append their record r behind the nin records already in rec, in lane order.  -> the new nin.
__device__ __forceinline__ int kp_compact(float4 *rec, const int nin, const bool inside, const float4 r) {
    const unsigned long long msk = __ballot(inside);
    if (inside) rec[nin + __popcll(msk & ((1ull << (threadIdx.x & 63)) - 1ull))] = r;
    return nin + __popcll(msk);
}

// 64 shadow records (1e18 away: influence exactly 0, row 0: finite data) behind the nin records, so the step loop needs no validity test
__device__ __forceinline__ void kp_shadow(float4 *rec, const int nin) {
    rec[nin + (threadIdx.x & 63)] = make_float4(1e18f, 0.f, 0.f, __int_as_float(0));
}

// The aggregation of ONE query m by one wave (see the file header): acc[ch][v] = MFMA accumulators (rows = kernel points,
// column j = channel c0 + ch*16*VEC + VEC*j + v), npos = neighbours whose feature row sums to > 0 (kpconv.py:113-114).
// rec = the wave's private LDS record buffer (PHASE + KP_PAD entries); a is a private copy (frame shift).
// SORTED (needs REC): the staging of the sorted prefix only, see KpArgs.  ONE_PHASE: the caller guarantees H <= PHASE - without the
// phase loop nothing of the staging is loop-carried, and the global-store kernels need 12 - 23 registers fewer than their unsorted forms
// (the fused kernel keeps the loop: without it its 32-channel form spills).
template <int VEC, int NCH, int PHASE, bool REC, bool SORTED = false, bool ONE_PHASE = false>
__device__ __forceinline__ void kp_aggregate_query(KpArgs a, const int m, const int c0, float4 *rec, f32x4 (&acc)[NCH][VEC], int &npos) {
    static_assert(REC || !SORTED, "the sorted form stages from records");
    constexpr int KP_PHASE = PHASE;
    const int lane = threadIdx.x & 63;
    const int j = lane & 15;
    kp_shift_frame<REC>(a, m);
    const KpQuery q = kp_query(a, m, j);
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch)
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[ch][v] = (f32x4){0.f, 0.f, 0.f, 0.f};
    npos = 0;
    const int32_t *irow = a.idx + (size_t)m * a.H;
    // per-lane channel byte offsets, clamped so that every load is unconditional (branch-free inner loop).  A lane whose
    // channels are out of range multiplies whatever it loaded into MFMA columns that are never stored; a shadow neighbour
    // has weight 0 (its record points at row 0, finite data).
    unsigned coffb[NCH];
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
        const int c = c0 + ch * 16 * VEC + VEC * j;
        coffb[ch] = c < a.C ? 4u * c : 0u;
    }
    const char *fbase = reinterpret_cast<const char *>(a.feats);
    const unsigned ldfb = 4u * a.ldf;
    [[maybe_unused]] bool done = false;   // SORTED: the row's survivors are all staged (wave-uniform)

    for (int h0 = 0; h0 < (ONE_PHASE ? 1 : a.H); h0 += KP_PHASE) {
        const int nh = a.H - h0 < KP_PHASE ? a.H - h0 : KP_PHASE;  // multiple of 4
        // ---- stage the records of this phase: lane = neighbour; all index loads first, then all gathers
        int idr[KP_PHASE / 64];
#pragma unroll
        for (int r = 0; r < KP_PHASE / 64; ++r) {
            const int hl = r * 64 + lane;
            idr[r] = irow[h0 + (hl < nh ? hl : 0)];
            if (hl >= nh) idr[r] = a.N;
        }
        int nin = 0;   // neighbours of this phase inside the kernel's support (wave-uniform)
        if constexpr (SORTED) {
            const KpStop stop = kp_stop(q);   // per phase, not across the step loop: it then costs the loop no registers
            const uint32_t *bits = kp_bits(a, m);   // (the frame shift leaves row_pos alone)
            unsigned fw[KP_PHASE / 64];   // the flag words of all neighbours: a few cache lines per wave, L1-resident
#pragma unroll
            for (int r = 0; r < KP_PHASE / 64; ++r) fw[r] = bits[(unsigned)idr[r] < (unsigned)a.N ? idr[r] >> 5 : 0];
#pragma unroll
            for (int r = 0; r < KP_PHASE / 64; ++r) {
                const bool valid = (unsigned)idr[r] < (unsigned)a.N;
                const unsigned long long vm = __ballot(valid);
                npos += __popcll(__ballot(valid && ((fw[r] >> (idr[r] & 31)) & 1u)));   // kpconv.py:113-115 counts over ALL neighbours
                if (!done && vm != 0) {   // wave-uniform
                    const int idc = valid ? idr[r] : 0;
                    float px = 0.f, py = 0.f, pz = 0.f;
                    int pos;
                    bool got = true;   // this lane's record is gathered
                    if (r == 0 && h0 == 0) {   // the row's first 16 neighbours, then - only if something behind them can be inside - the rest
                        got = lane < 16;
                        if (got) kp_support<REC>(a, idc, px, py, pz, pos);
                        const float ex = px - q.qx, ey = py - q.qy, ez = pz - q.qz;
                        done = !((vm >> 15) & 1) || kp_prefix_done(kp_lane_value((ex * ex + ey * ey) + ez * ez, 15), stop);
                        if (!done) {
                            if (!got) kp_support<REC>(a, idc, px, py, pz, pos);
                            got = true;
                        }
                    } else {
                        kp_support<REC>(a, idc, px, py, pz, pos);
                    }
                    // kpconv.py:93: neighbours centred on the query
                    const float dx = px - q.qx, dy = py - q.qy, dz = pz - q.qz;
                    const float d2 = (dx * dx + dy * dy) + dz * dz;
                    const bool inside = valid && got && d2 < q.rsup2;
                    nin = kp_compact(rec, nin, inside, make_float4(dx, dy, dz, __int_as_float(idr[r])));
                    if (!done) done = !((vm >> 63) & 1) || kp_prefix_done(kp_lane_value(d2, 63), stop);
                }
            }
        } else {
            float px[KP_PHASE / 64], py[KP_PHASE / 64], pz[KP_PHASE / 64];
            int pos[KP_PHASE / 64];
#pragma unroll
            for (int r = 0; r < KP_PHASE / 64; ++r) kp_support<REC>(a, (unsigned)idr[r] < (unsigned)a.N ? idr[r] : 0, px[r], py[r], pz[r], pos[r]);
#pragma unroll
            for (int r = 0; r < KP_PHASE / 64; ++r) {
                const bool valid = (unsigned)idr[r] < (unsigned)a.N;
                npos += __popcll(__ballot(valid && pos[r] != 0));   // kpconv.py:113-115 counts over ALL neighbours
                // kpconv.py:93: neighbours centred on the query
                const float dx = px[r] - q.qx, dy = py[r] - q.qy, dz = pz[r] - q.qz;
                const bool inside = valid && (dx * dx + dy * dy) + dz * dz < q.rsup2;
                nin = kp_compact(rec, nin, inside, make_float4(dx, dy, dz, __int_as_float(idr[r])));
            }
        }
        kp_shadow(rec, nin);
        __builtin_amdgcn_wave_barrier();
        kp_steps<VEC, NCH>(fbase, ldfb, coffb, rec, nin, q.kx, q.ky, q.kz, q.inv_sigma, acc);
        __builtin_amdgcn_wave_barrier();
    }
}

// The bf16 hi / lo planes (same rounding as the GEMM's on-the-fly split: identical products) of the VEC adjacent channels that a lane
// holds of accumulator row r, to hi and lo: VEC bf16 each, packed in pairs.
template <int VEC>
__device__ __forceinline__ void kp_split_store(const f32x4 (&acc)[VEC], const int r, uint16_t *hi_dst, uint16_t *lo_dst) {
    if constexpr (VEC == 4) {
        uint2 hi, lo;
        cofi_split2(acc[0][r], acc[1][r], hi.x, lo.x);
        cofi_split2(acc[2][r], acc[3][r], hi.y, lo.y);
        *reinterpret_cast<uint2 *>(hi_dst) = hi;
        *reinterpret_cast<uint2 *>(lo_dst) = lo;
    } else if constexpr (VEC == 2) {
        unsigned hi, lo;
        cofi_split2(acc[0][r], acc[1][r], hi, lo);
        *reinterpret_cast<unsigned *>(hi_dst) = hi;
        *reinterpret_cast<unsigned *>(lo_dst) = lo;
    } else {
        unsigned hi, lo;
        cofi_split2(acc[0][r], 0.f, hi, lo);
        hi_dst[0] = (uint16_t)hi;
        lo_dst[0] = (uint16_t)lo;
    }
}

// The store of one query's accumulators (channels from c0, see kp_aggregate_query) to row m of a.agg: fp32 (M, ld_agg), or with PLANES
// the bf16 hi plane (M, ld_agg bf16) and the lo plane a.planes_lo elements behind it.  CHECK_C: a.C may end inside this pass.
// The lane ids are taken HERE, after the step loop, so that nothing of the store addresses occupies registers across it.
template <int VEC, int NCH, bool CHECK_C, bool PLANES>
__device__ __forceinline__ void kp_store_rows(const KpArgs &a, const int m, const int c0, const f32x4 (&acc)[NCH][VEC]) {
    const int lane = __lane_id() & 63, j = lane & 15, g = lane >> 4;   // & 63: g <= 3 is known, three of the four k < 15 tests fold away
    // D layout 16x16: row (kernel point) = 4*g + r, col = j  ->  channels c .. c+VEC-1 contiguous
    float *orow = a.agg + (size_t)m * a.ld_agg;
    uint16_t *hrow = reinterpret_cast<uint16_t *>(a.agg) + (size_t)m * a.ld_agg;
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
        const int c = c0 + ch * 16 * VEC + VEC * j;
        if (!CHECK_C || c < a.C) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int k = 4 * g + r;
                if (k < 15) {
                    const size_t o = (size_t)k * a.C + c;
                    if constexpr (PLANES)
                        kp_split_store<VEC>(acc[ch], r, hrow + o, hrow + o + a.planes_lo);
                    else if constexpr (VEC == 4)
                        *reinterpret_cast<float4 *>(orow + o) = make_float4(acc[ch][0][r], acc[ch][1][r], acc[ch][2][r], acc[ch][3][r]);
                    else if constexpr (VEC == 2)
                        *reinterpret_cast<float2 *>(orow + o) = make_float2(acc[ch][0][r], acc[ch][1][r]);
                    else
                        orow[o] = acc[ch][0][r];
                }
            }
        }
    }
}

// kpconv.py:113-115: the divisor of a query with npos neighbours of positive feature sum, and its store for query m
__device__ __forceinline__ float kp_count(const int npos) { return (float)(npos > 1 ? npos : 1); }

__device__ __forceinline__ void kp_store_cnt(const KpArgs &a, const int m, const int npos) {
    if (__lane_id() == 0) a.cnt[m] = kp_count(npos);
}

// What a global-store kernel leaves of query m: its rows in the form a.planes_lo asks for and, from the wave with `first`, the count.
template <int VEC, int NCH, bool CHECK_C>
__device__ __forceinline__ void kp_store(const KpArgs &a, const int m, const int c0, const f32x4 (&acc)[NCH][VEC], const int npos, const bool first) {
    if (a.planes_lo)
        kp_store_rows<VEC, NCH, CHECK_C, true>(a, m, c0, acc);
    else
        kp_store_rows<VEC, NCH, CHECK_C, false>(a, m, c0, acc);
    if (first) kp_store_cnt(a, m, npos);
}

// amdgpu_waves_per_eu: the occupancy each form had before the step loop got its wave-uniform branches - left alone, the register
// allocator answers them with a second copy of the accumulators and loses a wave per SIMD (profiles/kpconv_records/README.md).
template <int VEC, int NCH, bool REC, bool SORTED = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(VEC * NCH == 8 ? 4 : (VEC * NCH == 4 ? 6 : 8)))) void kpconv_aggregate_kernel(KpArgs a) {
    __shared__ float4 rec_s[4][KP_PHASE_DEFAULT + KP_PAD];
    const int wv = threadIdx.x >> 6;
    // the query id is wave-uniform: keep it (and everything derived from it) in scalar registers
    int m = __builtin_amdgcn_readfirstlane(xcd_contiguous_block(blockIdx.x, gridDim.x) * 4 + wv);
    if (m >= a.M) return;
    if (a.order) m = (m / a.Mpf) * a.Mpf + a.order[m];
    const int c0 = blockIdx.y * (16 * VEC * NCH);
    f32x4 acc[NCH][VEC];
    int npos;
    kp_aggregate_query<VEC, NCH, KP_PHASE_DEFAULT, REC, SORTED, SORTED>(a, m, c0, rec_s[wv], acc, npos);   // sorted: the host sends H <= 128
    kp_store<VEC, NCH, true>(a, m, c0, acc, npos, blockIdx.y == 0);
}

// Wide layers (C = 256 / 512: NP = C / 128 channel passes) with few queries (1280 ... 2560 at the deep stages): the NP passes of a
// query are NP waves of ONE workgroup that stage its neighbour records TOGETHER - each wave a 1/NP share of the 128 neighbours,
// survivors concatenated in neighbour order through LDS - instead of every pass repeating the whole staging.  Same records, same
// order as kp_aggregate_query: identical bits.
template <int NP, bool REC>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(5))) void kpconv_aggregate_shared_kernel(KpArgs a) {
    constexpr int VEC = 4, NCH = 2, QW = 4 / NP, SH = 128 / NP;   // queries per workgroup, neighbours staged per wave
    __shared__ float4 rec_s[QW][128 + KP_PAD];
    __shared__ int cnt_s[QW][NP], pos_s[QW][NP];
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int qs = wv / NP, p = wv % NP;
    const int j = lane & 15;
    int m = __builtin_amdgcn_readfirstlane(xcd_contiguous_block(blockIdx.x, gridDim.x) * QW + qs);   // host: M % QW == 0
    if (a.order) m = (m / a.Mpf) * a.Mpf + a.order[m];
    kp_shift_frame<REC>(a, m);
    const KpQuery q = kp_query(a, m, j);
    // ---- this wave's share of the staging: neighbours [p * SH, (p + 1) * SH), lane = neighbour
    const int hl = p * SH + lane;
    const bool mine = lane < SH && hl < a.H;
    const int id = mine ? a.idx[(size_t)m * a.H + hl] : a.N;
    const bool valid = (unsigned)id < (unsigned)a.N;
    float px, py, pz;
    int rp;
    kp_support<REC>(a, valid ? id : 0, px, py, pz, rp);
    const float dx = px - q.qx, dy = py - q.qy, dz = pz - q.qz;
    const bool inside = valid && (dx * dx + dy * dy) + dz * dz < q.rsup2;
    const int nin_w = __popcll(__ballot(inside)), npos_w = __popcll(__ballot(valid && rp != 0));
    if (lane == 0) { cnt_s[qs][p] = nin_w; pos_s[qs][p] = npos_w; }
    __syncthreads();
    int off = 0, nin = 0, npos = 0;
#pragma unroll
    for (int w = 0; w < NP; ++w) {
        const int c = cnt_s[qs][w];
        off += w < p ? c : 0;
        nin += c;
        npos += pos_s[qs][w];
    }
    // wave-uniform, but read from LDS: into scalar registers, so that the step loop's tests on nin are scalar branches
    nin = __builtin_amdgcn_readfirstlane(nin);
    npos = __builtin_amdgcn_readfirstlane(npos);
    float4 *rec = rec_s[qs];
    kp_compact(rec, off, inside, make_float4(dx, dy, dz, __int_as_float(id)));   // behind the survivors of the waves before this one
    if (p == 0) kp_shadow(rec, nin);
    __syncthreads();
    // ---- this wave's channel pass over the shared records
    const int c0 = p * (16 * VEC * NCH);
    unsigned coffb[NCH];
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) coffb[ch] = 4u * (c0 + ch * 16 * VEC + VEC * j);
    f32x4 acc[NCH][VEC];
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch)
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[ch][v] = (f32x4){0.f, 0.f, 0.f, 0.f};
    kp_steps<VEC, NCH>(reinterpret_cast<const char *>(a.feats), 4u * a.ldf, coffb, rec, nin, q.kx, q.ky, q.kz, q.inv_sigma, acc);
    kp_store<VEC, NCH, false>(a, m, c0, acc, npos, p == 0);
}

// C <= 4 (the first layer of the encoder: [intensity | normal]).  What a neighbour costs in the staging is the number of distinct
// cache lines its data lies in (measured: without the separate position gathers the general kernel's 40 us for this layer drop to
// 29), so this layer reads ONE 32-byte record per neighbour, packed once per frame by kp_pack_c4_kernel: [f0 f1 f2 f3 | x y z | pos],
// pos = (f0 + .. + f3 > 0) (kpconv.py:113-114).  Lane = neighbour gathers the record, parks offset and features in LDS, and the MFMA
// chain (same operands, same order as the general kernel: identical bits) runs from LDS alone.
__global__ void kp_pack_c4_kernel(const float *feats, int ldf, int C, const float *pts, int N, float4 *out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const float *f = feats + (size_t)i * ldf, *p = pts + (size_t)i * 3;
    const float4 fv = make_float4(f[0], C > 1 ? f[1] : 0.f, C > 2 ? f[2] : 0.f, C > 3 ? f[3] : 0.f);
    const float sum = (fv.x + fv.z) + (fv.y + fv.w);   // the butterfly order of row_sum_positive_kernel (wave_sum) for C <= 4
    out[2 * (size_t)i] = fv;
    out[2 * (size_t)i + 1] = make_float4(p[0], p[1], p[2], sum > 0.0f ? 1.0f : 0.0f);
}

// SORTED: the two halves of a record are gathered for the sorted prefix of the row only, the flags come from a.bits (see KpArgs).
template <bool SORTED>
__global__ __launch_bounds__(256) void kpconv_aggregate_c4_kernel(KpArgs a) {   // a.feats = packed records (N, 8)
    constexpr int PH = 128;
    __shared__ float4 rec_s[4][PH + 4];   // + one step of shadow records behind the compacted list
    __shared__ float4 fea_s[4][PH + 4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int m = __builtin_amdgcn_readfirstlane(xcd_contiguous_block(blockIdx.x, gridDim.x) * 4 + wv);
    if (m >= a.M) return;
    if (a.order) m = (m / a.Mpf) * a.Mpf + a.order[m];
    const int j = lane & 15, g = lane >> 4;
    const float4 *recs = reinterpret_cast<const float4 *>(a.feats) + 2 * (size_t)(m / a.Mpf) * a.N;   // stack mode: this query's frame
    const KpQuery q = kp_query(a, m, j);   // the support of kp_aggregate_query: same neighbours kept, same order -> identical bits
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    int npos = 0;
    const int32_t *irow = a.idx + (size_t)m * a.H;
    float4 *rec = rec_s[wv], *fea = fea_s[wv];
    const float fmask = j < a.C ? 1.0f : 0.0f;           // MFMA columns past C multiply zeros
    const float *fsel = reinterpret_cast<const float *>(fea) + (j & 3);
    [[maybe_unused]] bool done = false;   // SORTED: the row's survivors are all staged (wave-uniform)
    for (int h0 = 0; h0 < a.H; h0 += PH) {
        const int nh = a.H - h0 < PH ? a.H - h0 : PH;    // multiple of 4
        int idr[2];
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int hl = r * 64 + lane;
            idr[r] = hl < nh ? irow[h0 + hl] : a.N;
        }
        int nin = 0;
        if constexpr (SORTED) {
            const uint32_t *bits = kp_bits(a, m);
            const KpStop stop = kp_stop(q);
            unsigned fw[2];
#pragma unroll
            for (int r = 0; r < 2; ++r) fw[r] = bits[(unsigned)idr[r] < (unsigned)a.N ? idr[r] >> 5 : 0];
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const bool valid = (unsigned)idr[r] < (unsigned)a.N;
                const unsigned long long vm = __ballot(valid);
                npos += __popcll(__ballot(valid && ((fw[r] >> (idr[r] & 31)) & 1u)));
                if (!done && vm != 0) {   // wave-uniform
                    const size_t idc = valid ? idr[r] : 0;
                    float4 f = make_float4(0.f, 0.f, 0.f, 0.f), p = f;
                    bool got = true;
                    if (r == 0 && h0 == 0) {   // the row's first 16 neighbours, then - only if something behind them can be inside - the rest
                        got = lane < 16;
                        if (got) { f = recs[2 * idc]; p = recs[2 * idc + 1]; }
                        const float ex = p.x - q.qx, ey = p.y - q.qy, ez = p.z - q.qz;
                        done = !((vm >> 15) & 1) || kp_prefix_done(kp_lane_value((ex * ex + ey * ey) + ez * ez, 15), stop);
                        if (!done) {
                            if (!got) { f = recs[2 * idc]; p = recs[2 * idc + 1]; }
                            got = true;
                        }
                    } else {
                        f = recs[2 * idc];
                        p = recs[2 * idc + 1];
                    }
                    const float dx = p.x - q.qx, dy = p.y - q.qy, dz = p.z - q.qz;
                    const float d2 = (dx * dx + dy * dy) + dz * dz;
                    const bool inside = valid && got && d2 < q.rsup2;
                    const unsigned long long msk = __ballot(inside);   // the two-array compaction of the unsorted form
                    if (inside) {
                        const int slot = nin + __popcll(msk & ((1ull << lane) - 1ull));
                        rec[slot] = make_float4(dx, dy, dz, 0.f);
                        fea[slot] = f;
                    }
                    nin += __popcll(msk);
                    if (!done) done = !((vm >> 63) & 1) || kp_prefix_done(kp_lane_value(d2, 63), stop);
                }
            }
        } else {
            float4 fr[2], pp[2];
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const int idc = (unsigned)idr[r] < (unsigned)a.N ? idr[r] : 0;
                fr[r] = recs[2 * (size_t)idc];
                pp[r] = recs[2 * (size_t)idc + 1];
            }
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const bool valid = (unsigned)idr[r] < (unsigned)a.N;
                npos += __popcll(__ballot(valid && pp[r].w != 0.f));
                const float dx = pp[r].x - q.qx, dy = pp[r].y - q.qy, dz = pp[r].z - q.qz;
                const bool inside = valid && (dx * dx + dy * dy) + dz * dz < q.rsup2;
                // kp_compact writes one array; two calls cost this kernel registers and instructions, so its two-array compaction stays here
                const unsigned long long msk = __ballot(inside);
                if (inside) {
                    const int slot = nin + __popcll(msk & ((1ull << lane) - 1ull));
                    rec[slot] = make_float4(dx, dy, dz, 0.f);
                    fea[slot] = fr[r];
                }
                nin += __popcll(msk);
            }
        }
        if (lane < 4) {   // the last step is filled up with shadow neighbours: influence exactly 0, zero features
            rec[nin + lane] = make_float4(1e18f, 0.f, 0.f, 0.f);
            fea[nin + lane] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        __builtin_amdgcn_wave_barrier();
        const int steps = (nin + 3) >> 2;
        for (int t = 0; t < steps; ++t) {
            const float4 rc = rec[4 * t + g];
            const float f = fsel[(4 * t + g) * 4] * fmask;
            const float dx = rc.x - q.kx, dy = rc.y - q.ky, dz = rc.z - q.kz;
            const float sq = (dx * dx + dy * dy) + dz * dz;
            const float w = fmaxf(1.0f - __builtin_amdgcn_sqrtf(sq) * q.inv_sigma, 0.0f);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w, f, acc, 0, 0, 0);
        }
        __builtin_amdgcn_wave_barrier();
    }
    if (j < a.C) {   // MFMA column j = channel j
        float *orow = a.agg + (size_t)m * a.ld_agg;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int k = 4 * g + r;
            if (k < 15) orow[(size_t)k * a.C + j] = acc[r];
        }
    }
    kp_store_cnt(a, m, npos);
}

// ---- KPConv as ONE kernel for the narrow layers (mid = 32 / 64 channels: the stages with 20 480 ... 5 120 queries) ----------------
// kpconv.py:91-116 end to end:  y[m] = (sum_k agg[m, k, :] W[k]) / max(#neighbours with positive feature sum, 1) + bias,
// plus the GroupNorm statistics partials of y.  The (M, 15 mid) aggregate - 39 MB per layer at these stages, written and read back
// by the two-kernel form - never leaves the CU:
//   a workgroup (8 waves) owns `qt` queries (= one statistics slab: 64 / 32 / 16 rows, so that a layer is >= 256 workgroups) and
//   works through them 16 at a time: every wave aggregates two queries exactly as kpconv_aggregate_kernel does and leaves their
//   (15 x mid) results as bf16 hi / lo planes in an LDS tile (16 x 15 mid); then the 8 waves multiply the tile with W
//   (pre-split bf16 planes streamed from L2, 3-term split on v_mfma_f32_16x16x32_bf16): wave = (16-column tile, K range), partial
//   tiles summed through LDS in a fixed order; epilogue: / count, + bias, store, column sums for the statistics.
// LDS 75 KB (mid 64, records staged 64 neighbours at a time) / 52 KB (mid 32): two workgroups per CU; the gather phase is
// bound by the texture-address unit, not by occupancy (measured: 16 waves per CU run it as fast as 28).
// MEASURED on MI355X (KITTI frame, us per launch, fused vs aggregate + GEMM): mid 32, 20 480 queries 58-91 vs ~65; mid 64, 10 240
// queries 63-87 vs ~52; whole forward 490 vs 503 frames/s.  A workgroup alternates between a gather phase (texture unit busy,
// matrix cores idle) and a GEMM phase (the opposite) with barriers in between, and 320-1280 such workgroups quantise badly on 256 CUs
// x 2 slots, while the two-kernel form spreads 20 480 independent one-wave queries evenly and its GEMM runs at full occupancy.  Kept
// as an opt-in (COFI_KPCONV_FUSED=1 in cofii2p_amd/kpfpn.py): it removes 2 x 39 MB of fabric traffic per layer, which matters once
// the frame is bandwidth-bound; not the default.
struct KpFusedArgs {
    KpArgs a;                       // agg / cnt / ld_agg unused
    const uint16_t *w_hi, *w_lo;    // bf16 planes of W, (mid rows, ldw), K index = kernel point * mid + channel
    int ldw;
    const float *bias;
    float *y;
    int ldy;
    float *colpart;                 // (M / qt, mid >> stat_shift, 2) or nullptr
    int stat_shift;
    int qt;                         // queries per workgroup = rows per statistics slab: 16, 32 or 64
};

template <int MID, int PHASE, bool RECS, bool SORTED = false>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4, 4))) void kpconv_fused_kernel(KpFusedArgs fa) {   // two workgroups per CU

    constexpr int VEC = MID / 16, K = 15 * MID, KLD = K + 8, NT = MID / 16, KQ = 8 / NT, KSTEPS = K / 32;
    constexpr int REC = PHASE + KP_PAD;
    constexpr int RG = 512 / MID;   // epilogue: thread = (column, row group); row groups
    constexpr int RPT = 16 / RG;    // rows per thread and 16-query step
    constexpr int PF = 4;           // k-steps of W fragments in flight per wave
    static_assert(REC * 16 >= 256 * 4, "the partial tiles alias the record buffers");
    __shared__ float4 rec_s[8][REC];
    __shared__ __attribute__((aligned(16))) uint16_t t_hi[16 * KLD];
    __shared__ __attribute__((aligned(16))) uint16_t t_lo[16 * KLD];
    __shared__ float cnt_s[16];
    __shared__ int m_s[16];
    float *part_s = reinterpret_cast<float *>(&rec_s[0][0]);   // [8][256]; live only inside the GEMM phase / the final fold
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int j = lane & 15, g = lane >> 4;
    const int b = xcd_contiguous_block(blockIdx.x, gridDim.x);
    const int en = tid % MID, erg = tid / MID;
    const float bias_n = fa.bias ? fa.bias[en] : 0.f;
    float cs = 0.f, cq = 0.f;
    // GEMM-phase role of this wave
    const int nt = wv % NT, kq = wv / NT;
    const int ks0 = kq * KSTEPS / KQ, ks1 = (kq + 1) * KSTEPS / KQ;
    const uint16_t *wh = fa.w_hi + (size_t)(nt * 16 + j) * fa.ldw + g * 8;
    const uint16_t *wl = fa.w_lo + (size_t)(nt * 16 + j) * fa.ldw + g * 8;
    const uint16_t *ah = t_hi + j * KLD + g * 8, *al = t_lo + j * KLD + g * 8;

    for (int st = 0; st < fa.qt; st += 16) {
        // ---- aggregation: two queries per wave
#pragma unroll 1
        for (int u = 0; u < 2; ++u) {
            const int ql = 2 * wv + u;
            const int pos = b * fa.qt + st + ql;
            int m = pos;
            if (fa.a.order) m = (pos / fa.a.Mpf) * fa.a.Mpf + fa.a.order[pos];
            m = __builtin_amdgcn_readfirstlane(m);
            f32x4 acc[1][VEC];
            int npos;
            kp_aggregate_query<VEC, 1, PHASE, RECS, SORTED>(fa.a, m, 0, rec_s[wv], acc, npos);
            // D layout 16x16: row (kernel point) = 4 g + r, column j -> channels VEC j .. VEC j + VEC - 1 of tile row ql
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int k = 4 * g + r;
                if (k < 15) {
                    const int off = ql * KLD + k * MID + VEC * j;
                    kp_split_store<VEC>(acc[0], r, t_hi + off, t_lo + off);
                }
            }
            if (lane == 0) {
                cnt_s[ql] = kp_count(npos);
                m_s[ql] = m;
            }
        }
        // ---- tile (16 x K) . W^T (K x MID): this wave's 16 columns over its K range; the first W fragments are requested before
        //      the barrier (they do not depend on the tile)
        f32x4 c = {0.f, 0.f, 0.f, 0.f};
        CofiFrag bh[PF], bl[PF];
#pragma unroll
        for (int i = 0; i < PF; ++i) {
            const int ks = ks0 + i < ks1 ? ks0 + i : ks1 - 1;
            bh[i].u = *reinterpret_cast<const uint4 *>(wh + ks * 32);
            bl[i].u = *reinterpret_cast<const uint4 *>(wl + ks * 32);
        }
        __syncthreads();
#pragma unroll 1
        for (int k0 = ks0; k0 < ks1; k0 += PF) {
            if (k0 != ks0) {
#pragma unroll
                for (int i = 0; i < PF; ++i) {
                    const int ks = k0 + i < ks1 ? k0 + i : ks1 - 1;
                    bh[i].u = *reinterpret_cast<const uint4 *>(wh + ks * 32);
                    bl[i].u = *reinterpret_cast<const uint4 *>(wl + ks * 32);
                }
            }
#pragma unroll
            for (int i = 0; i < PF; ++i) {
                if (k0 + i < ks1) {   // wave-uniform
                    CofiFrag fh, fl;
                    fh.u = *reinterpret_cast<const uint4 *>(ah + (k0 + i) * 32);
                    fl.u = *reinterpret_cast<const uint4 *>(al + (k0 + i) * 32);
                    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fl.v, bh[i].v, c, 0, 0, 0);
                    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fh.v, bl[i].v, c, 0, 0, 0);
                    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fh.v, bh[i].v, c, 0, 0, 0);
                }
            }
        }
        // D layout: column j, rows 4 g + r -> part_s[wave][row][column]
#pragma unroll
        for (int r = 0; r < 4; ++r) part_s[wv * 256 + (4 * g + r) * 16 + j] = c[r];
        __syncthreads();
        // ---- fold the K ranges (fixed order), / count, + bias, store, column sums
#pragma unroll
        for (int rr = 0; rr < RPT; ++rr) {
            const int q = erg * RPT + rr;
            float x = 0.f;
#pragma unroll
            for (int z = 0; z < KQ; ++z) x += part_s[(z * NT + (en >> 4)) * 256 + q * 16 + (en & 15)];
            x = x / cnt_s[q] + bias_n;
            fa.y[(size_t)m_s[q] * fa.ldy + en] = x;
            cs += x;
            cq += x * x;
        }
        __syncthreads();   // tile, records (= partial tiles), cnt_s / m_s are rewritten by the next step
    }
    if (fa.colpart) {
        part_s[(erg * MID + en) * 2] = cs;
        part_s[(erg * MID + en) * 2 + 1] = cq;
        __syncthreads();
        if (tid < MID) {
            float s = 0.f, q = 0.f;
            for (int p = 0; p < RG; ++p) {
                s += part_s[(p * MID + tid) * 2];
                q += part_s[(p * MID + tid) * 2 + 1];
            }
            // one table entry per 2^stat_shift adjacent columns (fp64 butterfly, fixed order), as the GEMM epilogue writes it
            double ds = s, dq = q;
            for (int o = 1; o < (1 << fa.stat_shift); o <<= 1) {
                ds += __shfl_xor(ds, o, 64);
                dq += __shfl_xor(dq, o, 64);
            }
            if ((tid & ((1 << fa.stat_shift) - 1)) == 0) {
                float *o = fa.colpart + ((size_t)b * (MID >> fa.stat_shift) + (tid >> fa.stat_shift)) * 2;
                o[0] = (float)ds;
                o[1] = (float)dq;
            }
        }
    }
}

// row_pos[n] = (sum_c feats[n,c] > 0); one wave per row (kpconv.py:113-114 applied per source row)
__global__ void row_sum_positive_kernel(const float *feats, int ld, int N, int C, uint8_t *row_pos) {
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;
    const int lane = threadIdx.x & 63;
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s += feats[(size_t)n * ld + c];
    s = wave_sum(s);
    if (lane == 0) row_pos[n] = s > 0.0f ? 1 : 0;
}

// rec[n] = (x, y, z, flag): the support record of the REC aggregation kernels for a caller that arrives without one.  The flag is
// row_sum_positive_kernel's, summed in the same order.
__global__ void kp_pack_support_kernel(const float *feats, int ld, int N, int C, const float *pts, float4 *rec) {
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;
    const int lane = threadIdx.x & 63;
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s += feats[(size_t)n * ld + c];
    s = wave_sum(s);
    if (lane == 0) {
        const float *p = pts + 3 * (size_t)n;
        rec[n] = make_float4(p[0], p[1], p[2], s > 0.0f ? 1.0f : 0.0f);
    }
}

// out[m,c] = max_h x[idx[m,h], c], zero row behind idx == N.  One wave per (query, 32-channel chunk):
// lane (g = l>>3, c4 = l&7) reads float4 #c4 of the chunk for neighbours h = 8i+g, so one load instruction
// fetches 8 neighbour rows x 128 contiguous bytes; the 8 lane groups are folded with 3 xor-shuffles.
// Chunks are the slow grid axis: all queries of one chunk run together and its source slice
// (N x 128 B <= 2.6 MB) stays resident in every XCD's 4 MB L2.
__global__ __launch_bounds__(256) void neighbor_maxpool_kernel(const float *x, int ldx, int N, int C, const int32_t *idx, int M,
                                                               int H, float *out, int ldo, int Mpf, const int32_t *order) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int m = xcd_contiguous_block(blockIdx.x, gridDim.x) * 4 + wv;
    if (m >= M) return;
    if (order) m = (m / Mpf) * Mpf + order[m];  // spatially sorted processing order (see KpArgs::order)
    x += (size_t)(m / Mpf) * N * ldx;  // stack mode: frame-local indices
    const int g = lane >> 3, c = blockIdx.y * 32 + (lane & 7) * 4;
    const int32_t *irow = idx + (size_t)m * H;
    float4 best = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
    const bool cin = c < C;
    const float *xc = x + (cin ? c : 0);
    // 64 neighbours per round: the index row is read once, coalesced (lane = neighbour), and handed to the 8 lane groups by
    // shuffle, so the only per-neighbour memory instruction is the 1-KB feature load (8 rows x 128 B); the 8 loads of a round
    // are issued back to back.  Shadow neighbours (idx == N) read row 0 and are replaced by the zero row afterwards.
    for (int h0 = 0; h0 < H; h0 += 64) {
        const int hl = h0 + lane;
        const int myid = hl < H ? irow[hl] : INT_MIN;   // INT_MIN: past the row (ignored); anything else outside [0,N): zero row
        float4 v[8];
        int ids[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            ids[i] = __shfl(myid, 8 * i + g, 64);
            const unsigned row = (unsigned)ids[i] < (unsigned)N ? ids[i] : 0;
            v[i] = *reinterpret_cast<const float4 *>(xc + (size_t)row * ldx);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const bool real = (unsigned)ids[i] < (unsigned)N;
            const float other = ids[i] == INT_MIN ? -INFINITY : 0.f;
            best.x = fmaxf(best.x, real ? v[i].x : other); best.y = fmaxf(best.y, real ? v[i].y : other);
            best.z = fmaxf(best.z, real ? v[i].z : other); best.w = fmaxf(best.w, real ? v[i].w : other);
        }
    }
#pragma unroll
    for (int o = 8; o < 64; o <<= 1) {
        best.x = fmaxf(best.x, __shfl_xor(best.x, o, 64));
        best.y = fmaxf(best.y, __shfl_xor(best.y, o, 64));
        best.z = fmaxf(best.z, __shfl_xor(best.z, o, 64));
        best.w = fmaxf(best.w, __shfl_xor(best.w, o, 64));
    }
    if (g == 0 && cin) *reinterpret_cast<float4 *>(out + (size_t)m * ldo + c) = best;
}

// The same max-pool for a source that fits one CU's LDS a few channels at a time (deep stages: few rows, many channels, every source
// row listed by ~64 queries).  One 16-wave workgroup owns (frame, group of CH channels, one of S query ranges): it loads the frame's
// N x CH slice ONCE, coalesced - no union of neighbour lists to find - behind it a zero row (N: every index outside [0, N)) and a -inf
// row (N + 1: positions past the end of an index row), and then serves all H neighbours of its queries from LDS.
//   lanes     CH / 4 lanes per query, each folds one float4 of channels over all H neighbours: no cross-lane reduction.
//   staging   per wave and pass, the index rows of its 64 / (CH / 4) queries, HC neighbours at a time, as BYTE OFFSETS into the slice
//             (range rule applied once per index, not once per channel quad); a wave reads what it wrote itself: no block barrier in
//             the loop.  A query's HC offsets are HC / 4 16-byte quads, quad k stored at k ^ swz(query), so that the 16 lanes that a
//             ds_read_b128 serves together (MI355X: lanes {0-3, 12-15, 20-27}, ...) read 16 different bank quads.
//   the fold  fmaxf from -inf in neighbour order: the maximum is exact in any order, so the bits are neighbor_maxpool_kernel's.
// `order` plays no part: a workgroup walks all queries of its range whatever their order.
constexpr int MPS_WAVES = 16, MPS_STAGE = 1024;   // waves per workgroup; staged offsets per wave (4 KB)

template <int CH, int ROWS>
__global__ __launch_bounds__(64 * MPS_WAVES) void neighbor_maxpool_slice_kernel(const float *x, int ldx, int N, int C, const int32_t *idx, int Mpf,
                                                                                int H, float *out, int ldo, int S, int G, int vec) {
    constexpr int LPQ = CH / 4;          // lanes per query
    constexpr int QW = 64 / LPQ;         // queries per wave and pass
    constexpr int HC = MPS_STAGE / QW;   // neighbours per staged chunk
    constexpr int HQ = HC / 4;           // 16-byte quads per staged index row
    __shared__ float4 slice[ROWS * LPQ];
    __shared__ int4 stage[MPS_WAVES][MPS_STAGE / 4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int b = xcd_contiguous_block(blockIdx.x, gridDim.x);   // the channel groups of a frame share lines of x and the index table: one XCD
    const int g = b % G, s = (b / G) % S, f = b / (G * S);
    const int c0 = g * CH;
    x += (size_t)f * N * ldx;
    idx += (size_t)f * Mpf * H;
    out += (size_t)f * Mpf * ldo;
    {   // the slice: rows 0 .. N-1, then the zero row and the -inf row
        const int quad = tid % LPQ, c = c0 + quad * 4;
        constexpr int RSTEP = 64 * MPS_WAVES / LPQ;
        if ((vec & 1) && c0 + CH <= C) {
#pragma unroll 4
            for (int r = tid / LPQ; r < N; r += RSTEP) slice[r * LPQ + quad] = *reinterpret_cast<const float4 *>(x + (size_t)r * ldx + c);
        } else {
            for (int r = tid / LPQ; r < N; r += RSTEP) {
                const float *p = x + (size_t)r * ldx;
                slice[r * LPQ + quad] = make_float4(c < C ? p[c] : 0.f, c + 1 < C ? p[c + 1] : 0.f, c + 2 < C ? p[c + 2] : 0.f, c + 3 < C ? p[c + 3] : 0.f);
            }
        }
        if (tid < 2 * LPQ) {
            const float v = tid < LPQ ? 0.f : -INFINITY;
            slice[N * LPQ + tid] = make_float4(v, v, v, v);
        }
    }
    __syncthreads();
    const int per = (Mpf + S - 1) / S, lo = s * per, hi = min(Mpf, lo + per);
    const int ql = lane / LPQ, quad = lane % LPQ, c = c0 + quad * 4;
    const int swz = (ql / (64 / HC)) & (HQ - 1);
    const char *sbase = reinterpret_cast<const char *>(slice) + quad * 16;
    int4 *st = stage[wv];
    // one chunk = HC neighbours of the pass's QW queries; the index loads of the next chunk are in flight while this one is folded
    // -> whether the chunk is FULL (wave-uniform): every query of the pass exists, every neighbour of the chunk too, 16-byte index loads -
    // four unconditional loads per lane now and no range tests on h when the offsets are written
    const int lane_off = (lane / HQ) * H + (lane % HQ) * 4;
    auto load = [&](int q0, int h0, int4 (&o)[4]) -> bool {   // 4 quads per lane, consecutive lanes on consecutive quads of an index row
        const bool full = (vec & 4) && h0 + HC <= H && q0 + QW <= hi;
        if (full) {
            const int32_t *p = idx + ((size_t)q0 * H + h0) + lane_off;
#pragma unroll
            for (int i = 0; i < 4; ++i) o[i] = *reinterpret_cast<const int4 *>(p + (size_t)(i * (64 / HQ)) * H);
            return true;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = i * 64 + lane, qs = e / HQ, h = h0 + (e % HQ) * 4;
            const bool live = q0 + qs < hi;   // a query past the range reads nothing (its lanes fold the zero row and store nothing)
            const int32_t *p = idx + (size_t)(q0 + qs) * H + h;
            o[i].x = live && h < H ? p[0] : -1;
            o[i].y = live && h + 1 < H ? p[1] : -1;
            o[i].z = live && h + 2 < H ? p[2] : -1;
            o[i].w = live && h + 3 < H ? p[3] : -1;
        }
        return false;
    };
    int4 o[4];
    int q0 = lo + wv * QW, h0 = 0;
    bool full = q0 < hi && load(q0, 0, o);
    float4 best = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
    while (q0 < hi) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // the previous chunk's reads are done before its offsets are replaced
        __builtin_amdgcn_wave_barrier();
        // anything outside [0, N) -> the zero row N; past the end of the index row -> the -inf row N + 1
        if (full) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int qs = (i * 64 + lane) / HQ, k = lane % HQ;
                st[qs * HQ + (k ^ ((qs / (64 / HC)) & (HQ - 1)))] =
                    make_int4((int)min((unsigned)o[i].x, (unsigned)N) * (CH * 4), (int)min((unsigned)o[i].y, (unsigned)N) * (CH * 4),
                              (int)min((unsigned)o[i].z, (unsigned)N) * (CH * 4), (int)min((unsigned)o[i].w, (unsigned)N) * (CH * 4));
            }
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int e = i * 64 + lane, qs = e / HQ, k = e % HQ, h = h0 + k * 4;
                int4 r;
                r.x = h < H ? (int)min((unsigned)o[i].x, (unsigned)N) : N + 1;
                r.y = h + 1 < H ? (int)min((unsigned)o[i].y, (unsigned)N) : N + 1;
                r.z = h + 2 < H ? (int)min((unsigned)o[i].z, (unsigned)N) : N + 1;
                r.w = h + 3 < H ? (int)min((unsigned)o[i].w, (unsigned)N) : N + 1;
                st[qs * HQ + (k ^ ((qs / (64 / HC)) & (HQ - 1)))] = make_int4(r.x * (CH * 4), r.y * (CH * 4), r.z * (CH * 4), r.w * (CH * 4));
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        int nq0 = q0, nh0 = h0 + HC;
        if (nh0 >= H) {
            nh0 = 0;
            nq0 += MPS_WAVES * QW;
        }
        full = nq0 < hi && load(nq0, nh0, o);
        const int nq = (min(HC, H - h0) + 3) >> 2;
        auto fold = [&](const int4 a) {
            const float4 v0 = *reinterpret_cast<const float4 *>(sbase + a.x), v1 = *reinterpret_cast<const float4 *>(sbase + a.y);
            const float4 v2 = *reinterpret_cast<const float4 *>(sbase + a.z), v3 = *reinterpret_cast<const float4 *>(sbase + a.w);
            best.x = fmaxf(fmaxf(best.x, v0.x), fmaxf(fmaxf(v1.x, v2.x), v3.x));
            best.y = fmaxf(fmaxf(best.y, v0.y), fmaxf(fmaxf(v1.y, v2.y), v3.y));
            best.z = fmaxf(fmaxf(best.z, v0.z), fmaxf(fmaxf(v1.z, v2.z), v3.z));
            best.w = fmaxf(fmaxf(best.w, v0.w), fmaxf(fmaxf(v1.w, v2.w), v3.w));
        };
        if (nq == HQ) {   // a full chunk: all offset quads first, then the row reads back to back - the waits are counted, not drained
            int4 a[HQ];
#pragma unroll
            for (int k = 0; k < HQ; ++k) a[k] = st[ql * HQ + (k ^ swz)];
#pragma unroll
            for (int k = 0; k < HQ; ++k) fold(a[k]);
        } else {
            for (int k = 0; k < nq; ++k) fold(st[ql * HQ + (k ^ swz)]);
        }
        if (nh0 == 0) {   // the pass's last chunk
            const int m = q0 + ql;
            if (m < hi) {
                float *po = out + (size_t)m * ldo;
                if ((vec & 2) && c + 4 <= C) {
                    *reinterpret_cast<float4 *>(po + c) = best;
                } else {
                    if (c < C) po[c] = best.x;
                    if (c + 1 < C) po[c + 1] = best.y;
                    if (c + 2 < C) po[c + 2] = best.z;
                    if (c + 3 < C) po[c + 3] = best.w;
                }
            }
            best = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
        }
        q0 = nq0;
        h0 = nh0;
    }
}

// out[m,:] = x[idx[m*idx_stride], :] (zero row for idx == N)
__global__ void gather_rows_kernel(const float *x, int ldx, int N, int C, const int32_t *idx, int idx_stride, int M, float *out,
                                   int ldo, int Mpf) {
    const int m = blockIdx.x;
    x += (size_t)(m / Mpf) * N * ldx;  // stack mode: frame-local indices
    const int id = idx[(size_t)m * idx_stride];
    const bool valid = (unsigned)id < (unsigned)N;
    const int c4 = C >> 2;
    if (((ldx | ldo | C) & 3) == 0) {
        for (int c = threadIdx.x; c < c4; c += blockDim.x) {
            float4 v = valid ? reinterpret_cast<const float4 *>(x + (size_t)id * ldx)[c] : make_float4(0, 0, 0, 0);
            reinterpret_cast<float4 *>(out + (size_t)m * ldo)[c] = v;
        }
    } else {
        for (int c = threadIdx.x; c < C; c += blockDim.x) out[(size_t)m * ldo + c] = valid ? x[(size_t)id * ldx + c] : 0.0f;
    }
}

}  // namespace

extern "C" int cofi_row_sum_positive(const float *feats, int ld, int N, int C, uint8_t *row_pos, cofi_stream_t stream) {
    if (!feats || !row_pos || N < 0 || C <= 0 || ld < C) return COFI_EINVAL;
    if (N == 0) return 0;
    hipLaunchKernelGGL(row_sum_positive_kernel, dim3(cofi_cdiv(N, 4)), dim3(256), 0, cofi_s(stream), feats, ld, N, C, row_pos);
    return cofi_launch_status();
}

extern "C" int cofi_kp_pack_support(const float *feats, int ldf, int N, int C, const float *points, float *records, cofi_stream_t stream) {
    if (!feats || !points || !records || N < 0 || C <= 0 || ldf < C || ((uintptr_t)records & 15)) return COFI_EINVAL;
    if (N == 0) return 0;
    hipLaunchKernelGGL(kp_pack_support_kernel, dim3(cofi_cdiv(N, 4)), dim3(256), 0, cofi_s(stream), feats, ldf, N, C, points, (float4 *)records);
    return cofi_launch_status();
}

// The operands every aggregation kernel takes, under the entry points' own names (M, N: rows per frame).  The support is s_pts + row_pos,
// or records, or neither (first-layer form: feats are the packed records); the fused kernel has no agg / cnt.
static KpArgs kp_args(const float *feats, int ldf, int N, int C, const float *q_pts, const float *s_pts, const uint8_t *row_pos, const float *records,
                      const int32_t *idx, int M, int H, const float *kernel_points, float sigma, float *agg, int ld_agg, int agg_planes, float *cnt,
                      int frames, const int32_t *order) {
    KpArgs a{};
    a.feats = feats; a.ldf = ldf; a.N = N; a.C = C;
    a.q_pts = q_pts; a.s_pts = s_pts; a.row_pos = row_pos; a.recs = (const float4 *)records;
    a.idx = idx; a.M = M * frames; a.Mpf = M; a.H = H;
    a.kp = kernel_points; a.sigma = sigma;
    a.agg = agg; a.ld_agg = ld_agg; a.planes_lo = agg_planes ? (size_t)M * frames * ld_agg : 0; a.cnt = cnt;
    a.order = order;
    return a;
}

// kp_steps forms a feature row's byte offset with one 24 x 24-bit multiply: row ids and 4 ldf below 2^24, the frame's features below 4 GiB
static int kp_check_support(int N, int ldf) {
    return ((size_t)N * ldf * 4 >= ((size_t)1 << 32) || N >= (1 << 24) || (size_t)ldf * 4 >= (1u << 24)) ? COFI_EUNSUPPORTED : 0;
}

// Shape checks and kernel choice of the aggregation; REC: the support arrives as 16-byte records (a.recs) instead of a.s_pts / a.row_pos.
template <bool REC, bool SORTED = false>
static int kp_aggregate_launch(const KpArgs &a, int agg_planes, int frames, cofi_stream_t stream) {
    const int N = a.N, C = a.C, M = a.M, H = a.H, ldf = a.ldf, ld_agg = a.ld_agg;   // M: the queries of all frames
    if (N <= 0 || C <= 0 || a.Mpf < 0 || H <= 0 || (H & 3) || ldf < C || ld_agg < 15 * C || !(a.sigma > 0.f) || frames <= 0) return COFI_EINVAL;
    if (agg_planes && ((ld_agg & 7) || (C & 3) || ((uintptr_t)a.agg & 15))) return COFI_EINVAL;
    if (int rc = kp_check_support(N, ldf)) return rc;
    if (M == 0) return 0;
    if constexpr (SORTED)
        if (H > KP_PHASE_DEFAULT) return kp_aggregate_launch<REC, false>(a, agg_planes, frames, stream);   // the sorted kernels stage one phase
    hipStream_t s = cofi_s(stream);
    const int mb = cofi_cdiv(M, 4);
    if ((C == 256 || C == 512) && (ldf & 3) == 0 && H <= 128 && M % (C == 256 ? 2 : 1) == 0) {
        if (C == 256)
            hipLaunchKernelGGL((kpconv_aggregate_shared_kernel<2, REC>), dim3(M / 2), dim3(256), 0, s, a);
        else
            hipLaunchKernelGGL((kpconv_aggregate_shared_kernel<4, REC>), dim3(M), dim3(256), 0, s, a);
    } else if ((C & 3) == 0 && (ldf & 3) == 0 && C >= 64) {
        if (C % 128 == 0)
            hipLaunchKernelGGL((kpconv_aggregate_kernel<4, 2, REC, SORTED>), dim3(mb, C / 128), dim3(256), 0, s, a);
        else
            hipLaunchKernelGGL((kpconv_aggregate_kernel<4, 1, REC, SORTED>), dim3(mb, cofi_cdiv(C, 64)), dim3(256), 0, s, a);
    } else if ((C & 1) == 0 && (ldf & 1) == 0 && C >= 32) {
        hipLaunchKernelGGL((kpconv_aggregate_kernel<2, 1, REC, SORTED>), dim3(mb, cofi_cdiv(C, 32)), dim3(256), 0, s, a);
    } else {
        hipLaunchKernelGGL((kpconv_aggregate_kernel<1, 1, REC, SORTED>), dim3(mb, cofi_cdiv(C, 16)), dim3(256), 0, s, a);
    }
    return cofi_launch_status();
}

extern "C" int cofi_kpconv_aggregate(const float *feats, int ldf, int N, int C, const float *q_pts, const float *s_pts,
                                     const int32_t *idx, int M, int H, const float *kernel_points, float sigma,
                                     const uint8_t *row_pos, float *agg, int ld_agg, int agg_planes, float *cnt, int frames, const int32_t *order,
                                     cofi_stream_t stream) {
    if (!feats || !q_pts || !s_pts || !idx || !kernel_points || !row_pos || !agg || !cnt) return COFI_EINVAL;
    return kp_aggregate_launch<false>(kp_args(feats, ldf, N, C, q_pts, s_pts, row_pos, nullptr, idx, M, H, kernel_points, sigma, agg, ld_agg, agg_planes,
                                              cnt, frames, order), agg_planes, frames, stream);
}

// cofi_kpconv_aggregate with the support as 16-byte records (x, y, z, flag) - (frames * N, 4) floats, written by the GroupNorm apply
// kernels or cofi_kp_pack_support - in place of s_pts and row_pos: same kernels, same results, one gather per neighbour in the staging.
extern "C" int cofi_kpconv_aggregate_rec(const float *feats, int ldf, int N, int C, const float *q_pts, const float *records,
                                         const int32_t *idx, int M, int H, const float *kernel_points, float sigma, float *agg, int ld_agg,
                                         int agg_planes, float *cnt, int frames, const int32_t *order, cofi_stream_t stream) {
    if (!feats || !q_pts || !records || !idx || !kernel_points || !agg || !cnt || ((uintptr_t)records & 15)) return COFI_EINVAL;
    return kp_aggregate_launch<true>(kp_args(feats, ldf, N, C, q_pts, nullptr, nullptr, records, idx, M, H, kernel_points, sigma, agg, ld_agg, agg_planes,
                                             cnt, frames, order), agg_planes, frames, stream);
}

// The flag bits of the SORTED forms from records of `stride` floats whose last float is the flag (4: support records, 8: first-layer
// records): (frames, cofi_kp_bits_words(N)) 32-bit words, bit n & 31 of word n >> 5 of a frame = flag of its row n, padding bits 0.
extern "C" int cofi_kp_bits_words(int N) { return N > 0 ? cofi_cdiv(N, 32) : 0; }

extern "C" int cofi_kp_pack_bits(const float *records, int stride, int N, int frames, uint32_t *bits, cofi_stream_t stream) {
    if (!records || !bits || N <= 0 || frames <= 0 || (stride != 4 && stride != 8)) return COFI_EINVAL;
    hipLaunchKernelGGL(kp_pack_bits_kernel, dim3(cofi_cdiv(N, 256), frames), dim3(256), 0, cofi_s(stream), records, stride, stride - 1, N,
                       cofi_kp_bits_words(N), bits);
    return cofi_launch_status();
}

// a with the flag bits of its N rows per frame in the place of row_pos (see KpArgs)
static KpArgs kp_with_bits(KpArgs a, const uint32_t *bits) {
    a.row_pos = reinterpret_cast<const uint8_t *>(bits);
    return a;
}

// cofi_kpconv_aggregate_rec for index tables whose rows are sorted (see KpArgs): the records of a row's sorted prefix are gathered,
// the flags of all its neighbours come from `bits` (cofi_kp_pack_bits of these records).  Same results, bit for bit, on every sorted
// table; undefined on any other.  The wide layers (C = 256 / 512) run cofi_kpconv_aggregate_rec's kernel.
extern "C" int cofi_kpconv_aggregate_rec_sorted(const float *feats, int ldf, int N, int C, const float *q_pts, const float *records,
                                                const uint32_t *bits, const int32_t *idx, int M, int H, const float *kernel_points, float sigma,
                                                float *agg, int ld_agg, int agg_planes, float *cnt, int frames, const int32_t *order,
                                                cofi_stream_t stream) {
    if (!feats || !q_pts || !records || !bits || !idx || !kernel_points || !agg || !cnt || ((uintptr_t)records & 15)) return COFI_EINVAL;
    return kp_aggregate_launch<true, true>(kp_with_bits(kp_args(feats, ldf, N, C, q_pts, nullptr, nullptr, records, idx, M, H, kernel_points, sigma, agg,
                                                                ld_agg, agg_planes, cnt, frames, order), bits), agg_planes, frames, stream);
}

// First-layer form (C <= 4): pack [features | position | positive-sum flag] into 32-byte records once, then aggregate from them.
extern "C" int cofi_kp_pack_c4(const float *feats, int ldf, int C, const float *points, int N, float *records, cofi_stream_t stream) {
    if (!feats || !points || !records || N <= 0 || C <= 0 || C > 4 || ldf < C || ((uintptr_t)records & 15)) return COFI_EINVAL;
    hipLaunchKernelGGL(kp_pack_c4_kernel, dim3(cofi_cdiv(N, 256)), dim3(256), 0, cofi_s(stream), feats, ldf, C, points, N, (float4 *)records);
    return cofi_launch_status();
}

// bits: the SORTED form with these flag bits, nullptr: the unsorted form
static int kp_c4_launch(const float *records, const uint32_t *bits, int N, int C, const float *q_pts, const int32_t *idx, int M, int H,
                        const float *kernel_points, float sigma, float *agg, int ld_agg, float *cnt, int frames, const int32_t *order,
                        cofi_stream_t stream) {
    if (!records || !q_pts || !idx || !kernel_points || !agg || !cnt || ((uintptr_t)records & 15)) return COFI_EINVAL;
    if (N <= 0 || C <= 0 || C > 4 || M < 0 || H <= 0 || (H & 3) || ld_agg < 15 * C || !(sigma > 0.f) || frames <= 0) return COFI_EINVAL;
    if (M == 0) return 0;
    const KpArgs a = kp_with_bits(kp_args(records, 8, N, C, q_pts, nullptr, nullptr, nullptr, idx, M, H, kernel_points, sigma, agg, ld_agg, 0, cnt,
                                          frames, order), bits);
    const dim3 grid(cofi_cdiv((long)M * frames, 4));
    if (bits)
        hipLaunchKernelGGL(kpconv_aggregate_c4_kernel<true>, grid, dim3(256), 0, cofi_s(stream), a);
    else
        hipLaunchKernelGGL(kpconv_aggregate_c4_kernel<false>, grid, dim3(256), 0, cofi_s(stream), a);
    return cofi_launch_status();
}

extern "C" int cofi_kpconv_aggregate_c4(const float *records, int N, int C, const float *q_pts, const int32_t *idx, int M, int H,
                                        const float *kernel_points, float sigma, float *agg, int ld_agg, float *cnt, int frames,
                                        const int32_t *order, cofi_stream_t stream) {
    return kp_c4_launch(records, nullptr, N, C, q_pts, idx, M, H, kernel_points, sigma, agg, ld_agg, cnt, frames, order, stream);
}

// cofi_kpconv_aggregate_c4 for sorted index tables, bits = cofi_kp_pack_bits(records, 8, ...): see cofi_kpconv_aggregate_rec_sorted
extern "C" int cofi_kpconv_aggregate_c4_sorted(const float *records, const uint32_t *bits, int N, int C, const float *q_pts, const int32_t *idx, int M,
                                               int H, const float *kernel_points, float sigma, float *agg, int ld_agg, float *cnt, int frames,
                                               const int32_t *order, cofi_stream_t stream) {
    if (!bits) return COFI_EINVAL;
    return kp_c4_launch(records, bits, N, C, q_pts, idx, M, H, kernel_points, sigma, agg, ld_agg, cnt, frames, order, stream);
}

// rows per statistics slab (= queries per workgroup) the fused kernel uses for M queries per frame: the largest of 64 / 32 / 16 that
// divides M and still gives >= 256 workgroups; 0 = shape not supported (use cofi_kpconv_aggregate + cofi_gemm_f32_fused)
extern "C" int cofi_kpconv_fused_slab_rows(int C, int M, int frames) {
    if ((C != 32 && C != 64) || M <= 0 || frames <= 0 || (M % 16)) return 0;
    for (int q = 64; q >= 32; q >>= 1)
        if (M % q == 0 && (long)M * frames / q >= 256) return q;
    return 16;
}

template <bool REC, bool SORTED = false>
static int kp_fused_launch(const KpArgs &a, const void *w_planes, int ldw, const float *bias, float *y, int ldy, float *colpart, int stat_width,
                           int frames, cofi_stream_t stream) {
    const int N = a.N, C = a.C, M = a.Mpf, ldf = a.ldf;
    if (N <= 0 || M <= 0 || a.H <= 0 || (a.H & 3) || ldf < C || ldy < C || !(a.sigma > 0.f) || frames <= 0) return COFI_EINVAL;
    if (ldw < 15 * C || (ldw & 7) || ((uintptr_t)w_planes & 15)) return COFI_EINVAL;
    const int qt = cofi_kpconv_fused_slab_rows(C, M, frames);
    if (qt == 0 || (ldf & (C / 16 - 1))) return COFI_EUNSUPPORTED;
    if (int rc = kp_check_support(N, ldf)) return rc;
    int shift = 0;
    if (colpart) {
        if (stat_width <= 0 || (stat_width & (stat_width - 1)) || stat_width > 16 || (C % stat_width)) return COFI_EINVAL;
        while ((1 << shift) < stat_width) ++shift;
    }
    KpFusedArgs fa{};
    fa.a = a;
    fa.w_hi = (const uint16_t *)w_planes;
    fa.w_lo = fa.w_hi + (size_t)C * ldw;
    fa.ldw = ldw; fa.bias = bias; fa.y = y; fa.ldy = ldy; fa.colpart = colpart; fa.stat_shift = shift; fa.qt = qt;
    const int nwg = (int)((long)M * frames / qt);
    if (C == 64)
        hipLaunchKernelGGL((kpconv_fused_kernel<64, 64, REC, SORTED>), dim3(nwg), dim3(512), 0, cofi_s(stream), fa);
    else
        hipLaunchKernelGGL((kpconv_fused_kernel<32, 128, REC, SORTED>), dim3(nwg), dim3(512), 0, cofi_s(stream), fa);
    return cofi_launch_status();
}

extern "C" int cofi_kpconv_fused(const float *feats, int ldf, int N, int C, const float *q_pts, const float *s_pts, const int32_t *idx, int M, int H,
                                 const float *kernel_points, float sigma, const uint8_t *row_pos, const void *w_planes, int ldw, const float *bias,
                                 float *y, int ldy, float *colpart, int stat_width, int frames, const int32_t *order, cofi_stream_t stream) {
    if (!feats || !q_pts || !s_pts || !idx || !kernel_points || !row_pos || !w_planes || !y) return COFI_EINVAL;
    return kp_fused_launch<false>(kp_args(feats, ldf, N, C, q_pts, s_pts, row_pos, nullptr, idx, M, H, kernel_points, sigma, nullptr, 0, 0, nullptr, frames,
                                          order), w_planes, ldw, bias, y, ldy, colpart, stat_width, frames, stream);
}

// cofi_kpconv_fused with the support as 16-byte records (see cofi_kpconv_aggregate_rec)
extern "C" int cofi_kpconv_fused_rec(const float *feats, int ldf, int N, int C, const float *q_pts, const float *records, const int32_t *idx, int M,
                                     int H, const float *kernel_points, float sigma, const void *w_planes, int ldw, const float *bias, float *y,
                                     int ldy, float *colpart, int stat_width, int frames, const int32_t *order, cofi_stream_t stream) {
    if (!feats || !q_pts || !records || !idx || !kernel_points || !w_planes || !y || ((uintptr_t)records & 15)) return COFI_EINVAL;
    return kp_fused_launch<true>(kp_args(feats, ldf, N, C, q_pts, nullptr, nullptr, records, idx, M, H, kernel_points, sigma, nullptr, 0, 0, nullptr, frames,
                                         order), w_planes, ldw, bias, y, ldy, colpart, stat_width, frames, stream);
}

// cofi_kpconv_fused_rec for sorted index tables (see cofi_kpconv_aggregate_rec_sorted)
extern "C" int cofi_kpconv_fused_rec_sorted(const float *feats, int ldf, int N, int C, const float *q_pts, const float *records, const uint32_t *bits,
                                            const int32_t *idx, int M, int H, const float *kernel_points, float sigma, const void *w_planes, int ldw,
                                            const float *bias, float *y, int ldy, float *colpart, int stat_width, int frames, const int32_t *order,
                                            cofi_stream_t stream) {
    if (!feats || !q_pts || !records || !bits || !idx || !kernel_points || !w_planes || !y || ((uintptr_t)records & 15)) return COFI_EINVAL;
    return kp_fused_launch<true, true>(kp_with_bits(kp_args(feats, ldf, N, C, q_pts, nullptr, nullptr, records, idx, M, H, kernel_points, sigma, nullptr, 0,
                                                            0, nullptr, frames, order), bits), w_planes, ldw, bias, y, ldy, colpart, stat_width, frames,
                                       stream);
}

extern "C" int cofi_neighbor_maxpool(const float *x, int ldx, int N, int C, const int32_t *idx, int M, int H, float *out, int ldo,
                                     int frames, const int32_t *order, cofi_stream_t stream) {
    if (!x || !idx || !out || N <= 0 || C <= 0 || M < 0 || H <= 0 || ldx < C || ldo < C) return COFI_EINVAL;
    if ((C & 3) || (ldx & 3) || (ldo & 3) || ((uintptr_t)x & 15) || ((uintptr_t)out & 15)) return COFI_EINVAL;
    if (M == 0) return 0;
    if (frames <= 0) return COFI_EINVAL;
    hipLaunchKernelGGL(neighbor_maxpool_kernel, dim3(cofi_cdiv(M * frames, 4), cofi_cdiv(C, 32)), dim3(256), 0, cofi_s(stream), x, ldx, N,
                       C, idx, M * frames, H, out, ldo, M, order);
    return cofi_launch_status();
}

// The slice form: N source rows + the zero row + the -inf row at 8 channels (3072 rows) or 4 channels (6144 rows) of fp32 in 96 KB, next to
// the 64 KB of staged offsets.  0: the slice does not fit at 4 channels.
constexpr int MPS_ROWS8 = 3072, MPS_ROWS4 = 6144;
static int mps_channels(int N, int C) { return N + 2 <= MPS_ROWS8 && C > 4 ? 8 : (N + 2 <= MPS_ROWS4 ? 4 : 0); }

extern "C" int cofi_neighbor_maxpool_slice_ok(int N, int C, int H, int frames) {
    return N > 0 && C > 0 && H > 0 && frames > 0 && mps_channels(N, C) != 0;
}

extern "C" int cofi_neighbor_maxpool_slice(const float *x, int ldx, int N, int C, const int32_t *idx, int M, int H, float *out, int ldo,
                                           int frames, const int32_t *order, cofi_stream_t stream) {
    (void)order;   // a workgroup serves every query of its range from one slice: the processing order plays no part
    if (!x || !idx || !out || N <= 0 || C <= 0 || M < 0 || H <= 0 || ldx < C || ldo < C || frames <= 0) return COFI_EINVAL;
    const int ch = mps_channels(N, C);
    if (ch == 0) return COFI_EUNSUPPORTED;
    if (M == 0) return 0;
    const int G = cofi_cdiv(C, ch), passes = cofi_cdiv(M, MPS_WAVES * (256 / ch));
    if ((long)frames * G * passes >= (1L << 31)) return COFI_EUNSUPPORTED;
    // few frames: split a frame's queries over S workgroups per channel group, down to one pass per wave, until the chip is covered twice
    const int S = std::max(1, std::min(passes, 512 / (frames * G)));
    const int vec = ((ldx & 3) == 0 && ((uintptr_t)x & 15) == 0 ? 1 : 0) | ((ldo & 3) == 0 && ((uintptr_t)out & 15) == 0 ? 2 : 0) |
                    ((H & 3) == 0 && ((uintptr_t)idx & 15) == 0 ? 4 : 0);
    if (ch == 8)
        hipLaunchKernelGGL((neighbor_maxpool_slice_kernel<8, MPS_ROWS8>), dim3(frames * G * S), dim3(64 * MPS_WAVES), 0, cofi_s(stream), x, ldx, N, C,
                           idx, M, H, out, ldo, S, G, vec);
    else
        hipLaunchKernelGGL((neighbor_maxpool_slice_kernel<4, MPS_ROWS4>), dim3(frames * G * S), dim3(64 * MPS_WAVES), 0, cofi_s(stream), x, ldx, N, C,
                           idx, M, H, out, ldo, S, G, vec);
    return cofi_launch_status();
}

extern "C" int cofi_gather_rows(const float *x, int ldx, int N, int C, const int32_t *idx, int idx_stride, int M, float *out,
                                int ldo, int frames, cofi_stream_t stream) {
    if (!x || !idx || !out || N <= 0 || C <= 0 || M < 0 || idx_stride <= 0 || ldx < C || ldo < C) return COFI_EINVAL;
    if (M == 0) return 0;
    if (frames <= 0) return COFI_EINVAL;
    hipLaunchKernelGGL(gather_rows_kernel, dim3(M * frames), dim3(C >= 1024 ? 256 : (C >= 256 ? 128 : 64)), 0, cofi_s(stream), x, ldx, N,
                       C, idx, idx_stride, M * frames, out, ldo, M);
    return cofi_launch_status();
}
