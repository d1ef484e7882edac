// Dense fp32 contraction on v_mfma_f32_32x32x2_f32 (exact fp32, 157 TF/s chip peak) with fused epilogues.
//   C[m,n] = act( (sum_k A[m,k] * W[n,k]) / rowdiv[m] + bias[n] )                (plain)
//   C[m,:] = relu?( LayerNorm_n( ... ) * gamma + beta ) + res[m,:]               (fused LayerNorm, N <= 128)
//   colpart[slab, n] = { sum_m C[m,n], sum_m C[m,n]^2 } over the rows of a slab   (fused column statistics:
//        feeds stack-mode GroupNorm / InstanceNorm / the token-axis Q normalisation without another pass)
// Both operands are K-contiguous ("NT"): activations row-major, weights in nn.Linear's (N,K) layout — no
// packing of the reference's Linear weights is needed.
//
// Tile: BM x BN x 32 per workgroup of 4 waves (2x2), each wave TM x TN MFMA tiles of 32x32.
// LDS image: rows of 32 k-values padded to 36 floats.  A lane reads its MFMA operands as ONE
// ds_read_b128 per 4 MFMA steps: lane (i = l&31, h = l>>5) reads k = 8c+4h .. 8c+4h+3 of row i and
// uses element e in step (c,e).  The k-order seen by the MFMA chain is therefore a permutation
// (step (c,e) contracts k = 8c+e and 8c+4+e), identical for A and W, which a sum does not care
// about.  Row stride 36 dwords makes the b128 reads (16-lane groups, bank = dword mod 64) and the
// b128 staging writes (8-lane groups, bank mod 32) conflict free (MI355X_MICROARCH §LDS).
//
// Epilogue: the accumulator tile goes through LDS once (the operand buffers are dead by then), so rows
// are written back as whole 128-B+ segments by consecutive lanes and the row / column reductions of the
// fused epilogues are plain shuffles over row-major data.
//
// Deep-K / small-MN problems are split over K (gridDim.z) into a workspace and reduced in fixed
// order by splitk_epilogue_kernel (same row-wise epilogue): deterministic, no float atomics.
#include "common.h"
#include "stat_fold.h"
#include <stdio.h>
#include <stdlib.h>
#include <type_traits>

namespace {

constexpr int BK = 32;
constexpr int LDS_LD = 36;

struct GemmArgs {
    const float *A, *W;
    float *C;
    const float *bias, *rowdiv;
    float *ws;
    float *colpart;                    // optional (nslab, N, 2)
    const float *ln_gamma, *ln_beta;   // optional fused LayerNorm over the N columns of a row
    const float *res;                  // optional residual added after the LayerNorm
    // optional row index of the residual (cofi_gemm_f32_fused_res): output row m of frame f = m / res_out_rows takes residual row
    // f * res_rows + res_idx[m * res_idx_stride]; an index outside [0, res_rows) is a shadow point, its residual is zero (res_src_row)
    const int32_t *res_idx;
    int res_idx_stride, res_rows, res_out_rows;
    int lda, ldw, ldc, ldr, M, N, K, act, ksplit, kchunk, ln_relu;
    float ln_eps;
    int bf16x3;
    int wsplit;        // W is pre-split: W points at the bf16 hi plane (rows of ldw bf16), the lo plane starts w_lo_off elements later
    long w_lo_off;
    int asplit;        // A is pre-split as well (dense GEMM only): A points at the bf16 hi plane (M rows of lda bf16), lo plane a_lo_off elements later
    long a_lo_off;
    // implicit-GEMM convolution (cv_ks > 0): A is an NHWC map (H*W rows of lda floats), row m of the GEMM is
    // output pixel (m / Wo, m % Wo), column k is (tap = k / Cin, channel = k % Cin); K = ks*ks*Cin
    int cv_ks, cv_H, cv_W, cv_Cin, cv_Wo, cv_stride, cv_pad;
    int cv_Pout;  // output pixels per frame (stack mode: GEMM row m is frame m / cv_Pout, pixel m % cv_Pout)
    int xcd;      // 0: hardware tile order; 1 + log2(gridDim.x): XCD-contiguous tile order (gemm_block_id)
    unsigned xcd_rcp_gy;
    int l2n;          // COFI_GEMM_L2NORM: rows are L2-normalised after bias / residual / activation (a tile spans the whole row, N <= 128)
    int act_col0;     // the activation applies to output columns >= act_col0 only (two layers sharing one A operand: [skip | conv1])
    int stat_shift;   // colpart holds one entry per 2^stat_shift adjacent columns: (nslab, N >> stat_shift, 2)
    // pending normalisation of the A operand (stat_fold.h): the loader applies  a -> leaky(a * sc[c] + sh[c])  to every element
    // it stages, c = column of a dense A / input channel of a convolution; an.part == nullptr: none.  an_rows = GEMM rows per
    // frame (tiles never straddle frames: host-checked).
    NormSrc an;
    int an_rows;
    int f16;          // COFI_GEMM_F16X3: a launch that takes the 256 x 128 kernel runs gemm_f16_big_kernel (three fp16 products) instead of the six-product one
    const float *wscale;  // COFI_GEMM_W_F16PRE: the panel scales of the pre-split W (one per 128 rows), stored behind the (N, ldw) matrix; nullptr: W is fp32
    unsigned *fixflags;   // ... one word per workgroup of that launch, behind the split-K partials in the workspace: 1 = the repair launch computes this tile
    int dbg;          // cofi_tune_big_debug (include/cofi_hip_tune.h) of the calling thread; 0 on the product path.  Bit 64: the generic row-wise epilogue instead of the straight-line one (same bits)
};

// Tile coordinates of this workgroup.  The dispatcher hands workgroup L (x fastest, then y, then the K-split slice z) to XCD
// L % 8, so with e.g. 8 column tiles every XCD owns ONE column of tiles and pulls the whole A operand through its private L2
// (8x the algorithmic traffic).  xcd = 1 + log2(gridDim.x) re-numbers the workgroups so that each XCD works through one
// CONTIGUOUS eighth of that order: the column tiles of a row panel of A run on the same XCD at the same time and A crosses the
// fabric once; with split-K an XCD works on (part of) ONE K-slice and reads only that slice of W.
// Power-of-two gridDim.x and an exact multiply-high reciprocal of gridDim.y: no division in the prologue of latency-bound launches.
struct BlockId { int x, y, z; };
__device__ __forceinline__ BlockId gemm_block_id(const GemmArgs &g) {
    if (!g.xcd) return {(int)blockIdx.x, (int)blockIdx.y, (int)blockIdx.z};
    const int sh = g.xcd - 1, gy = gridDim.y, nblk = (gy * (int)gridDim.z) << sh;
    const int l = ((blockIdx.z * gy + blockIdx.y) << sh) + blockIdx.x;
    const int q = nblk >> 3, r = nblk & 7, c = l & 7, i = l >> 3;   // bijective for any block count
    const int t = (c < r ? c * (q + 1) : r * (q + 1) + (c - r) * q) + i;
    const int yz = t >> sh;
    const int z = g.xcd_rcp_gy ? (int)__umulhi((unsigned)yz, g.xcd_rcp_gy) : yz;   // rcp = ceil(2^32 / gy), exact for yz, gy < 2^16; 0: gy = 1
    return {t & ((1 << sh) - 1), yz - z * gy, z};
}

// A-operand tile loader shared by both MFMA kernels: float4 number j of this thread covers row m0 + lrow + 32j,
// k .. k+3.  Dense: A[row, k].  Convolution: the input pixel under tap k / Cin of output pixel `row`, zero
// outside the image (Cin % 4 == 0, so a float4 never straddles two taps).
template <int A_LD4>
struct ATileLoader {
    int yo[A_LD4], xo[A_LD4], fb[A_LD4];  // output pixel coordinates and first input row of the frame
    __device__ __forceinline__ void init(const GemmArgs &g, int m0, int lrow) {
        if (g.cv_ks) {
#pragma unroll
            for (int j = 0; j < A_LD4; ++j) {
                const int r = min(m0 + lrow + 32 * j, g.M - 1);
                const int f = r / g.cv_Pout, pix = r - f * g.cv_Pout;
                fb[j] = f * g.cv_H * g.cv_W;
                yo[j] = pix / g.cv_Wo;
                xo[j] = pix - yo[j] * g.cv_Wo;
            }
        }
    }
    // Every load is UNCONDITIONAL on a clamped (always valid) address and masked afterwards with a select: predicated
    // loads compile to one exec-masked basic block each, which stops the scheduler from batching the loads of a tile
    // and puts an s_waitcnt vmcnt(0) behind every one of them.
    __device__ __forceinline__ void load(const GemmArgs &g, int m0, int lrow, int k, bool kin, float4 (&ra)[A_LD4]) const {
        const float4 zero = make_float4(0, 0, 0, 0);
        const int kc = kin ? k : 0;
        if (g.cv_ks == 0) {
#pragma unroll
            for (int j = 0; j < A_LD4; ++j) {
                const int r = m0 + lrow + 32 * j;
                const float4 v = *reinterpret_cast<const float4 *>(g.A + (size_t)min(r, g.M - 1) * g.lda + kc);
                ra[j] = (kin && r < g.M) ? v : zero;
            }
        } else {
            const int tap = kc / g.cv_Cin, c = kc - tap * g.cv_Cin;
            const int dy = tap / g.cv_ks, dx = tap - dy * g.cv_ks;
#pragma unroll
            for (int j = 0; j < A_LD4; ++j) {
                const int r = m0 + lrow + 32 * j;
                const int yi = yo[j] * g.cv_stride - g.cv_pad + dy, xi = xo[j] * g.cv_stride - g.cv_pad + dx;
                const bool ok = kin && r < g.M && (unsigned)yi < (unsigned)g.cv_H && (unsigned)xi < (unsigned)g.cv_W;
                const int yc = min(max(yi, 0), g.cv_H - 1), xc = min(max(xi, 0), g.cv_W - 1);
                const float4 v = *reinterpret_cast<const float4 *>(g.A + ((size_t)fb[j] + (size_t)yc * g.cv_W + xc) * g.lda + c);
                ra[j] = ok ? v : zero;
            }
        }
    }
};

__device__ __forceinline__ float apply_act(float v, int act) {
    if (act == COFI_ACT_RELU) return fmaxf(v, 0.0f);
    if (act == COFI_ACT_SIGMOID) return 1.0f / (1.0f + expf(-v));
    if (act == COFI_ACT_LEAKY01) return v >= 0.0f ? v : v * 0.1f;
    return v;
}

// apply_act for a workgroup-UNIFORM activation code: ReLU / LeakyReLU are computed branch-free and chosen with scalar-condition
// selects; only the sigmoid (score heads) sits behind a - uniform - branch.  Same expressions as apply_act: identical bits.
__device__ __forceinline__ float apply_act_uniform(float v, int act) {
    if (act == COFI_ACT_SIGMOID) return 1.0f / (1.0f + expf(-v));
    const float relu = fmaxf(v, 0.0f), leaky = v >= 0.0f ? v : v * 0.1f;
    return act == COFI_ACT_RELU ? relu : (act == COFI_ACT_LEAKY01 ? leaky : v);
}

// Column statistics of a slab: fold the per-thread sums of the RPP row phases in a fixed order (deterministic).  red = (RPP, BN, 2) floats
// of LDS that every thread has finished reading (the caller's barrier); all threads of the workgroup call.  One barrier inside.
template <int BN, int RPP>
__device__ __forceinline__ void colstat_fold(const GemmArgs &g, float *red, const float (&cs)[4], const float (&cq)[4], int slab, int n0, int tr, int tc) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        red[(tr * BN + 4 * tc + e) * 2 + 0] = cs[e];
        red[(tr * BN + 4 * tc + e) * 2 + 1] = cq[e];
    }
    __syncthreads();
    if (threadIdx.x < BN && n0 + (int)threadIdx.x < g.N) {
        float s = 0.f, q = 0.f;
        for (int p = 0; p < RPP; ++p) {
            s += red[(p * BN + threadIdx.x) * 2 + 0];
            q += red[(p * BN + threadIdx.x) * 2 + 1];
        }
        if (g.stat_shift) {
            // one table entry per 2^stat_shift adjacent columns (<= BN, aligned: a group never leaves the tile, and N is a
            // multiple of the width, so the lanes of a group are all active): fp64 butterfly, fixed order
            double ds = s, dq = q;
            for (int o = 1; o < (1 << g.stat_shift); o <<= 1) {
                ds += __shfl_xor(ds, o, 64);
                dq += __shfl_xor(dq, o, 64);
            }
            if ((threadIdx.x & ((1u << g.stat_shift) - 1)) == 0) {
                float *o = g.colpart + ((size_t)slab * (g.N >> g.stat_shift) + ((n0 + threadIdx.x) >> g.stat_shift)) * 2;
                o[0] = (float)ds;
                o[1] = (float)dq;
            }
        } else {
            float *o = g.colpart + ((size_t)slab * g.N + n0 + threadIdx.x) * 2;
            o[0] = s;
            o[1] = q;
        }
    }
}

// Residual source row of output row `row` (< M).  No index table: the row itself.  With one (GemmArgs::res_idx): frame-local, as
// gather_rows_kernel; for a shadow index row 0 of the frame is addressed (always valid) and `ok` comes back false - the caller puts zeros
// in its place.
__device__ __forceinline__ int res_src_row(const GemmArgs &g, int row, bool &ok) {
    ok = true;
    if (!g.res_idx) return row;   // uniform
    const int src = g.res_idx[(size_t)row * g.res_idx_stride];
    ok = (unsigned)src < (unsigned)g.res_rows;
    return (row / g.res_out_rows) * g.res_rows + (ok ? src : 0);   // < frames * res_rows (host-checked to fit an int)
}

// The residual rows of one 64-row slab for the lean epilogues of the 256 x 128 kernels: dst[p] = residual of row row0 + p * RPP, columns
// col .. col + 3 (one float4: the caller checked ldr % 4 and the base alignment).  Rows past M read the clamped row M - 1 - they are never
// stored - and, with an index table, the index of that clamped row (the table has M entries); a shadow index gives zeros.
template <int NP, int RPP>
__device__ __forceinline__ void load_res_slab(const GemmArgs &g, int row0, int col, float (&dst)[NP][4]) {
    if (g.res_idx) {   // uniform
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            bool ok;
            const int src = res_src_row(g, min(row0 + p * RPP, g.M - 1), ok);
            const f32x4 t = *reinterpret_cast<const f32x4 *>(g.res + (size_t)src * g.ldr + col);
#pragma unroll
            for (int e = 0; e < 4; ++e) dst[p][e] = ok ? t[e] : 0.f;
        }
    } else {
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const f32x4 t = *reinterpret_cast<const f32x4 *>(g.res + (size_t)min(row0 + p * RPP, g.M - 1) * g.ldr + col);
#pragma unroll
            for (int e = 0; e < 4; ++e) dst[p][e] = t[e];
        }
    }
}

// The straight-line form of the row-wise epilogue (no fused LayerNorm / L2 normalisation, whole float4 columns inside N, aligned output):
// x[p][e] = value of row row0 + p * RPP, column col + e.  Every option is a workgroup-uniform scalar and guards a whole BLOCK of the
// NP x 4 elements (a guard around a single element gets if-converted: the compiler then runs e.g. the 10-instruction division for every
// element and selects afterwards - measured: 20 us of epilogue for one 256 x 128 tile, 4500 cycles per 64-row slab).  Same operations in
// the same order per element as the generic path: identical bits.
template <int NP, int RPP, bool RES>
__device__ __forceinline__ void epi_fast_apply(const GemmArgs &g, float (&x)[NP][4], const float (&bias4)[4], const float (&rd)[NP],
                                               const float (&rs)[NP][4], int col, int row0, float (&cs)[4], float (&cq)[4]) {
    if (g.rowdiv) {
#pragma unroll
        for (int p = 0; p < NP; ++p)
#pragma unroll
            for (int e = 0; e < 4; ++e) x[p][e] = x[p][e] / rd[p];
    }
#pragma unroll
    for (int p = 0; p < NP; ++p)
#pragma unroll
        for (int e = 0; e < 4; ++e) x[p][e] = (x[p][e] + bias4[e]) + (RES ? rs[p][e] : 0.f);   // residual before the activation; the zero keeps -0.0 + 0.0 = +0.0 of the generic path
    const int act = g.act;
    if (act != COFI_ACT_NONE) {
        bool on[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) on[e] = col + e >= g.act_col0;
        if (act == COFI_ACT_RELU) {
#pragma unroll
            for (int p = 0; p < NP; ++p)
#pragma unroll
                for (int e = 0; e < 4; ++e) x[p][e] = on[e] ? fmaxf(x[p][e], 0.0f) : x[p][e];
        } else if (act == COFI_ACT_LEAKY01) {
#pragma unroll
            for (int p = 0; p < NP; ++p)
#pragma unroll
                for (int e = 0; e < 4; ++e) x[p][e] = (on[e] && !(x[p][e] >= 0.0f)) ? x[p][e] * 0.1f : x[p][e];
        } else {
#pragma unroll
            for (int p = 0; p < NP; ++p)
#pragma unroll
                for (int e = 0; e < 4; ++e) x[p][e] = on[e] ? 1.0f / (1.0f + expf(-x[p][e])) : x[p][e];
        }
    }
    if (g.colpart) {
#pragma unroll
        for (int p = 0; p < NP; ++p)
            if (row0 + p * RPP < g.M) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    cs[e] += x[p][e];
                    cq[e] += x[p][e] * x[p][e];
                }
            }
    }
#pragma unroll
    for (int p = 0; p < NP; ++p)
        if (row0 + p * RPP < g.M) *reinterpret_cast<float4 *>(g.C + (size_t)(row0 + p * RPP) * g.ldc + col) = make_float4(x[p][0], x[p][1], x[p][2], x[p][3]);
}

// Row-wise epilogue over a ROWS x BN tile held row-major in LDS (`tile`, leading dimension TLD) or summed
// from split-K partials.  Thread (tr, tc): row phase tr, float4 column chunk tc.  NT threads.
// The operands it reads from global memory come in two groups that a caller working through several slabs of one tile may load AHEAD:
// column-indexed parameters (EpiCols: once per tile) and row-indexed ones (EpiRows: per slab).  vmcnt counts stores too, so a load
// issued behind the stores of the previous slab makes its consumer wait for those stores' round trip: a multi-slab epilogue issues the
// next slab's loads before the current slab's stores (gemm_x6_big_kernel).
struct EpiCols { float bias4[4], gam4[4], bet4[4]; };
template <int NP> struct EpiRows { float rs[NP][4], rd[NP]; };

template <int BN>
__device__ __forceinline__ EpiCols epi_load_cols(const GemmArgs &g, int n0) {
    constexpr int TPR = BN / 4;
    const int col = n0 + 4 * ((int)threadIdx.x % TPR);
    EpiCols c;
#pragma unroll
    for (int e = 0; e < 4; ++e) { c.bias4[e] = 0.f; c.gam4[e] = 1.f; c.bet4[e] = 0.f; }
    if (!g.bias && !g.ln_gamma) return c;   // uniform
    if (n0 + BN <= g.N) {                   // uniform: no column tail in this tile
        if (g.bias) {
#pragma unroll
            for (int e = 0; e < 4; ++e) c.bias4[e] = g.bias[col + e];
        }
        if (g.ln_gamma) {
#pragma unroll
            for (int e = 0; e < 4; ++e) { c.gam4[e] = g.ln_gamma[col + e]; c.bet4[e] = g.ln_beta[col + e]; }
        }
        return c;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if (col + e < g.N) {
            if (g.bias) c.bias4[e] = g.bias[col + e];
            if (g.ln_gamma) { c.gam4[e] = g.ln_gamma[col + e]; c.bet4[e] = g.ln_beta[col + e]; }
        }
    }
    return c;
}

template <int ROWS, int BN, int NT>
__device__ __forceinline__ EpiRows<ROWS / (NT / (BN / 4))> epi_load_rows(const GemmArgs &g, int m0, int n0) {
    constexpr int TPR = BN / 4, RPP = NT / TPR, NP = ROWS / RPP;
    const int tc = threadIdx.x % TPR, tr = threadIdx.x / TPR;
    const int col = n0 + 4 * tc;
    const bool res_vec = g.res && ((g.ldr & 3) == 0) && ((reinterpret_cast<uintptr_t>(g.res) & 15) == 0) && col + 3 < g.N;
    EpiRows<NP> r;
    if (!g.rowdiv && !g.res) {   // uniform: nothing to load
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            r.rd[p] = 1.0f;
#pragma unroll
            for (int e = 0; e < 4; ++e) r.rs[p][e] = 0.f;
        }
        return r;
    }
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const int row = m0 + p * RPP + tr;
        const bool rin = row < g.M;
        r.rd[p] = (g.rowdiv && rin) ? g.rowdiv[row] : 1.0f;
#pragma unroll
        for (int e = 0; e < 4; ++e) r.rs[p][e] = 0.f;
        if (g.res && rin) {
            bool rok;
            const float *rp = g.res + (size_t)res_src_row(g, row, rok) * g.ldr + col;
            if (!rok) {   // shadow index: the zeros above
            } else if (res_vec) {
                const float4 t = *reinterpret_cast<const float4 *>(rp);
                r.rs[p][0] = t.x; r.rs[p][1] = t.y; r.rs[p][2] = t.z; r.rs[p][3] = t.w;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (col + e < g.N) r.rs[p][e] = rp[e];
            }
        }
    }
    return r;
}

template <int ROWS, int BN, bool FROM_WS, int NT = 256>
__device__ __forceinline__ void rowwise_epilogue_pre(const GemmArgs &g, const float *tile, int TLD, int m0, int n0, int slab, float *red,
                                                     const EpiCols &ec, const EpiRows<ROWS / (NT / (BN / 4))> &er) {
    constexpr int TPR = BN / 4;        // threads per row
    constexpr int RPP = NT / TPR;      // rows per pass
    constexpr int NP = ROWS / RPP;     // passes
    const int tc = threadIdx.x % TPR, tr = threadIdx.x / TPR;
    const int col = n0 + 4 * tc;
    const bool vec_ok = ((g.N & 3) == 0) && ((g.ldc & 3) == 0) && ((reinterpret_cast<uintptr_t>(g.C) & 15) == 0);
    float cs[4] = {0.f, 0.f, 0.f, 0.f}, cq[4] = {0.f, 0.f, 0.f, 0.f};
    const float (&bias4)[4] = ec.bias4, (&gam4)[4] = ec.gam4, (&bet4)[4] = ec.bet4;
    const float (&rs)[NP][4] = er.rs, (&rd)[NP] = er.rd;
    // phase 1: the tile values of all passes (split-K: every partial load of all passes is independent, so their latencies overlap)
    const bool fast = !g.ln_gamma && !g.l2n && vec_ok && n0 + BN <= g.N && !(g.dbg & 64);   // dbg 64 (tools only): the generic path
    float v[NP][4];
    if (FROM_WS || !fast) {
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const int rl = p * RPP + tr, row = m0 + rl;
        const bool rin = row < g.M;
        if constexpr (FROM_WS) {
            v[p][0] = v[p][1] = v[p][2] = v[p][3] = 0.f;
            if (rin) {
                const size_t total = (size_t)g.M * g.N;
                for (int z = 0; z < g.ksplit; ++z) {
                    const float *q = g.ws + (size_t)z * total + (size_t)row * g.N + col;
                    if ((g.N & 3) == 0 && col < g.N) {
                        const float4 t = *reinterpret_cast<const float4 *>(q);
                        v[p][0] += t.x; v[p][1] += t.y; v[p][2] += t.z; v[p][3] += t.w;
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (col + e < g.N) v[p][e] += q[e];
                    }
                }
            }
        } else {
            const float4 t = *reinterpret_cast<const float4 *>(tile + rl * TLD + 4 * tc);
            v[p][0] = t.x; v[p][1] = t.y; v[p][2] = t.z; v[p][3] = t.w;
        }
    }
    }
    // phase 2: arithmetic + stores.
    // FAST PATH - no fused LayerNorm / L2 normalisation, whole float4 columns inside N, aligned output: every decision is taken ONCE per
    // workgroup (uniform scalars), the loops below are straight-line code.  The generic path further down decides per element and costs
    // ~10 000 cycles per 64-row slab (measured on MI355X: 20 us of epilogue for one 256 x 128 tile), which was most of a short-K launch.
    // Same operations in the same order as the generic path: identical bits.
    if (fast) {
        // two passes at a time: blocks large enough not to be if-converted, small enough for the register budget of the kernels that
        // rely on two or three workgroups per CU (all NP x 4 values in flight through every stage cost them a workgroup); a tile in LDS
        // is read chunk by chunk
        constexpr int CH = NP >= 2 ? 2 : 1;
#pragma unroll
        for (int c = 0; c < NP / CH; ++c) {
            if constexpr (!FROM_WS) {
#pragma unroll
                for (int p = c * CH; p < (c + 1) * CH; ++p) {
                    const float4 t = *reinterpret_cast<const float4 *>(tile + (p * RPP + tr) * TLD + 4 * tc);
                    v[p][0] = t.x; v[p][1] = t.y; v[p][2] = t.z; v[p][3] = t.w;
                }
            }
            float (&vx)[CH][4] = reinterpret_cast<float (&)[CH][4]>(v[c * CH]);
            const float (&rdx)[CH] = reinterpret_cast<const float (&)[CH]>(rd[c * CH]);
            const float (&rsx)[CH][4] = reinterpret_cast<const float (&)[CH][4]>(rs[c * CH]);
            if (g.res) epi_fast_apply<CH, RPP, true>(g, vx, bias4, rdx, rsx, col, m0 + tr + c * CH * RPP, cs, cq);
            else epi_fast_apply<CH, RPP, false>(g, vx, bias4, rdx, rsx, col, m0 + tr + c * CH * RPP, cs, cq);
        }
    } else {
    // generic path (fused LayerNorm / L2 normalisation, column tails).  The row divisor guards the whole block of NP x 4 elements: around a
    // single element the branch is if-converted and the 10-instruction division runs for every element of every launch
    if (g.rowdiv) {
#pragma unroll
        for (int p = 0; p < NP; ++p)
#pragma unroll
            for (int e = 0; e < 4; ++e) v[p][e] = v[p][e] / rd[p];
    }
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const int row = m0 + p * RPP + tr;
        const bool rin = row < g.M;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[p][e] = v[p][e] + bias4[e];
        if (g.ln_gamma) {
            // LayerNorm over the N (<= BN) columns of this row: the TPR threads of a row are adjacent lanes
            float s = 0.f;
#pragma unroll
            for (int e = 0; e < 4; ++e) s += (col + e < g.N) ? v[p][e] : 0.f;
#pragma unroll
            for (int o = 1; o < TPR; o <<= 1) s += __shfl_xor(s, o, 64);
            const float mean = s / (float)g.N;
            float q = 0.f;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float d = v[p][e] - mean;
                q += (col + e < g.N) ? d * d : 0.f;
            }
#pragma unroll
            for (int o = 1; o < TPR; o <<= 1) q += __shfl_xor(q, o, 64);
            const float rstd = 1.0f / sqrtf(q / (float)g.N + g.ln_eps);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float x = (v[p][e] - mean) * rstd * gam4[e] + bet4[e];
                if (g.ln_relu) x = fmaxf(x, 0.f);
                v[p][e] = x + rs[p][e];
            }
        } else {
            // residual before the activation.  The activation code is workgroup-uniform, the columns it applies to (>= act_col0) are
            // a per-lane mask: a select, not a per-element divergent branch (three exec-masked regions per element made this loop
            // the longest part of a short-K launch)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float x = v[p][e] + rs[p][e];
                v[p][e] = (col + e >= g.act_col0) ? apply_act_uniform(x, g.act) : x;
            }
            if (g.l2n) {   // F.normalize(row, dim = 1): x / max(|x|, 1e-12); the TPR threads of a row are adjacent lanes
                float q = 0.f;
#pragma unroll
                for (int e = 0; e < 4; ++e) q += (col + e < g.N) ? v[p][e] * v[p][e] : 0.f;
#pragma unroll
                for (int o = 1; o < TPR; o <<= 1) q += __shfl_xor(q, o, 64);
                const float inv = 1.0f / fmaxf(sqrtf(q), 1e-12f);
#pragma unroll
                for (int e = 0; e < 4; ++e) v[p][e] *= inv;
            }
        }
        if (rin) {
            if (g.colpart) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    cs[e] += v[p][e];
                    cq[e] += v[p][e] * v[p][e];
                }
            }
            float *dst = g.C + (size_t)row * g.ldc + col;
            if (vec_ok && col + 3 < g.N) {
                *reinterpret_cast<float4 *>(dst) = make_float4(v[p][0], v[p][1], v[p][2], v[p][3]);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (col + e < g.N) dst[e] = v[p][e];
            }
        }
    }
    }
    if (g.colpart) {
        __syncthreads();
        colstat_fold<BN, RPP>(g, red, cs, cq, slab, n0, tr, tc);
    }
}

template <int ROWS, int BN, bool FROM_WS, int NT = 256>
__device__ __forceinline__ void rowwise_epilogue(const GemmArgs &g, const float *tile, int TLD, int m0, int n0, int slab, float *red) {
    const EpiCols ec = epi_load_cols<BN>(g, n0);
    const auto er = epi_load_rows<ROWS, BN, NT>(g, m0, n0);
    rowwise_epilogue_pre<ROWS, BN, FROM_WS, NT>(g, tile, TLD, m0, n0, slab, red, ec, er);
}

// ------------------------------------------------------------------------------------------------------
// The tail of gemm_planes_kernel and gemm_f16_big_kernel: what happens behind the K loop.  (gemm_kernel and gemm_bf16x3_kernel above / below
// and gemm_x6_big_kernel in gemm_x6_big.inc end in copies of their own of the same code: calling the shared form from them measured
// 0.2 - 0.8 % slower over their probes - 1 - 13 % per launch for the ANORM / CONV instantiations of gemm_x6_big_kernel -, outside the
// parent's run-to-run range: profiles/gemm_tail/README.md.  A change to the lean slab loop below has to be made in gemm_x6_big.inc as well.)
// Both hold the result as 32 x 32 MFMA tiles acc[TM][TN] in a wave grid, wave (wm, wn) owning rows
// wm * 32 TM .. and columns wn * 32 TN .. of the tile at (m0, n0); lane (li = lane & 31, lh = lane >> 5) holds in acc[i][j][r] the element
// at row (r & 3) + 8 * (r >> 2) + 4 * lh, column li of its 32 x 32 tile (the D layout).  `lds` is the workgroup's operand storage, re-used
// as a row-major fp32 slab of leading dimension BN + 4 (and as the scratch of the column-statistics fold).

// split-K: raw partial sums straight from the D layout into slice z of the workspace
template <int TM, int TN>
__device__ __forceinline__ void mfma32_store_partial(const GemmArgs &g, const f32x16 (&acc)[TM][TN], int z, int m0, int n0, int wm, int wn, int li, int lh) {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int col = n0 + wn * 32 * TN + j * 32 + li;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = m0 + wm * 32 * TM + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                if (row < g.M && col < g.N) g.ws[((size_t)z * g.M + row) * g.N + col] = acc[i][j][r];
            }
        }
}

// the 32-row blocks of 64-row slab h of the tile -> row-major LDS slab (waves that hold none of them write nothing)
template <int BN, int TM, int TN>
__device__ __forceinline__ void mfma32_slab_to_lds(const f32x16 (&acc)[TM][TN], float *lds, int h, int wm, int wn, int li, int lh) {
    constexpr int TLD = BN + 4;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int rb = wm * TM + i;   // 32-row block of the tile held in acc[i][*]
        if ((rb >> 1) == h) {
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int rl = (rb & 1) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                    lds[rl * TLD + wn * 32 * TN + j * 32 + li] = acc[i][j][r];
                }
        }
    }
}

// Tail of the kernels whose K loop does not end on a barrier (gemm_planes_kernel: LEAN = false; gemm_f16_big_kernel: LEAN = true),
// NT threads, 64-row slabs: split-K partial store, else the lean slab loop when its conditions hold, else barrier + generic
// slab loop.
template <int BM, int BN, int TM, int TN, int NT, bool LEAN>
__device__ __forceinline__ void mfma32_tile_tail(const GemmArgs &g, const f32x16 (&acc)[TM][TN], float *lds, int z, int m0, int n0,
                                                 int wm, int wn, int li, int lh, int tid) {
    static_assert(BM % 64 == 0, "64-row slabs");
    constexpr int TLD = BN + 4;
    if (g.ksplit > 1) {
        mfma32_store_partial<TM, TN>(g, acc, z, m0, n0, wm, wn, li, lh);
        return;
    }
    // LEAN epilogue (no fused LayerNorm / L2 normalisation / sigmoid, whole float4 columns inside N, aligned output - every launch of the
    // forward that takes the f16x3 kernel): straight-line code per slab, every decision uniform and taken once.  vmcnt counts stores as well
    // as loads: a load issued behind the stores of a slab makes its consumer wait for their round trip (and a wait the compiler places on a
    // path that happens to have no load at all still drains the stores) - four store round trips per tile otherwise.  So: bias and the row
    // divisors of the whole tile are loaded BEFORE the slab loop, which then holds no load at all; only a residual is loaded per slab, one
    // slab ahead of its use (before the stores of the slab in between).  Same operations in the same order as rowwise_epilogue: same bits.
    if constexpr (LEAN) {
    const bool vec_ok = ((g.N & 3) == 0) && ((g.ldc & 3) == 0) && ((reinterpret_cast<uintptr_t>(g.C) & 15) == 0);
    const bool res_ok = !g.res || (((g.ldr & 3) == 0) && ((reinterpret_cast<uintptr_t>(g.res) & 15) == 0));
    if (!g.ln_gamma && !g.l2n && vec_ok && res_ok && n0 + BN <= g.N && g.act != COFI_ACT_SIGMOID) {
        constexpr int TPR = BN / 4, RPP = NT / TPR, NP = 64 / RPP, NS = BM / 64;   // 256 threads, BN = 128: 32 threads per row, 8 rows per pass, 8 passes per slab
        const int tc = tid % TPR, tr = tid / TPR;
        const int col = n0 + 4 * tc;
        const bool has_stats = g.colpart != nullptr;
        float bias4[4] = {0.f, 0.f, 0.f, 0.f};
        if (g.bias) {
#pragma unroll
            for (int e = 0; e < 4; ++e) bias4[e] = g.bias[col + e];
        }
        float rd[NS][NP];
#pragma unroll
        for (int h = 0; h < NS; ++h)
#pragma unroll
            for (int p = 0; p < NP; ++p) rd[h][p] = 1.0f;
        if (g.rowdiv) {
#pragma unroll
            for (int h = 0; h < NS; ++h)
#pragma unroll
                for (int p = 0; p < NP; ++p) rd[h][p] = g.rowdiv[min(m0 + 64 * h + p * RPP + tr, g.M - 1)];   // rows past M are never stored
        }
        auto run = [&](auto with_res) __attribute__((always_inline)) {
            constexpr bool RES = decltype(with_res)::value;
            float rs[NP][4], rs_next[NP][4];
#pragma unroll
            for (int p = 0; p < NP; ++p)
#pragma unroll
                for (int e = 0; e < 4; ++e) rs[p][e] = rs_next[p][e] = 0.f;
            auto load_res = [&](int h, float (&dst)[NP][4]) __attribute__((always_inline)) {
                if constexpr (RES) load_res_slab<NP, RPP>(g, m0 + 64 * h + tr, col, dst);
            };
            load_res(0, rs);
            __syncthreads();   // every wave is done with the operand stages
#pragma unroll
            for (int h = 0; h < NS; ++h) {
                const bool live = m0 + 64 * h < g.M;   // uniform: no statistics slab (and no rows) behind the last valid row
                if (live) mfma32_slab_to_lds<BN, TM, TN>(acc, lds, h, wm, wn, li, lh);
                __syncthreads();
                if (h + 1 < NS) load_res(h + 1, rs_next);
                float cs[4] = {0.f, 0.f, 0.f, 0.f}, cq[4] = {0.f, 0.f, 0.f, 0.f};
                if (live) {
                    float x[NP][4];
#pragma unroll
                    for (int p = 0; p < NP; ++p) {
                        const f32x4 t = *reinterpret_cast<const f32x4 *>(lds + (p * RPP + tr) * TLD + 4 * tc);
#pragma unroll
                        for (int e = 0; e < 4; ++e) x[p][e] = t[e];
                    }
                    epi_fast_apply<NP, RPP, RES>(g, x, bias4, rd[h], rs, col, m0 + 64 * h + tr, cs, cq);
                }
                // every thread passes the same number of barriers whether the slab is live or dead: colstat_fold holds one, the dead
                // branch pairs it
                if (has_stats) {   // uniform.  Fold of the RPP row phases in a fixed order, as rowwise_epilogue
                    __syncthreads();
                    if (live) colstat_fold<BN, RPP>(g, lds, cs, cq, (m0 >> 6) + h, n0, tr, tc);
                    else __syncthreads();
                }
                __syncthreads();
                if constexpr (RES) {
#pragma unroll
                    for (int p = 0; p < NP; ++p)
#pragma unroll
                        for (int e = 0; e < 4; ++e) rs[p][e] = rs_next[p][e];
                }
            }
        };
        if (g.res) run(std::true_type{});
        else run(std::false_type{});
        return;
    }
    }
    // generic path: rowwise_epilogue per slab (loads its own operands); the stages are dead after the barrier
    __syncthreads();
#pragma unroll
    for (int h = 0; h < BM / 64; ++h) {
        if (m0 + 64 * h >= g.M) break;   // uniform: no statistics slab (and no rows) behind the last valid row
        mfma32_slab_to_lds<BN, TM, TN>(acc, lds, h, wm, wn, li, lh);
        __syncthreads();
        rowwise_epilogue<64, BN, false, NT>(g, lds, TLD, m0 + 64 * h, n0, (m0 >> 6) + h, lds);
        __syncthreads();
    }
}

template <int BM, int BN, int TM, int TN>
__global__ __launch_bounds__(256) void gemm_kernel(GemmArgs g) {
    static_assert(BM == 64 * TM && BN == 64 * TN, "2x2 waves");
    constexpr int A_LD4 = BM / 32;  // float4 loads per thread for the A tile
    constexpr int W_LD4 = BN / 32;
    constexpr int TLD = BN + 4;     // epilogue tile leading dimension
    static_assert(BM * TLD <= 2 * (BM + BN) * LDS_LD && (256 / (BN / 4)) * BN * 2 <= BM * TLD, "epilogue tile must fit in the operand buffers");
    __shared__ __attribute__((aligned(16))) float lds[2 * (BM + BN) * LDS_LD];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const BlockId bid = gemm_block_id(g);
    const int m0 = bid.y * BM, n0 = bid.x * BN;
    const int kbeg = bid.z * g.kchunk;
    const int kend = min(g.K, kbeg + g.kchunk);
    const int ntiles = (kend - kbeg + BK - 1) / BK;

    const int lrow = tid >> 3, lk = (tid & 7) * 4;  // staging map: 8 lanes cover one 128-B row slice
    float4 ra[A_LD4], rw[W_LD4];
    ATileLoader<A_LD4> aload;
    aload.init(g, m0, lrow);

    auto gload = [&](int t) {
        const int k = kbeg + t * BK + lk;
        const bool kin = k < kend;
        aload.load(g, m0, lrow, k, kin, ra);
#pragma unroll
        for (int j = 0; j < W_LD4; ++j) {
            const int r = n0 + lrow + 32 * j;
            const float4 v = *reinterpret_cast<const float4 *>(g.W + (size_t)min(r, g.N - 1) * g.ldw + (kin ? k : 0));
            rw[j] = (kin && r < g.N) ? v : make_float4(0, 0, 0, 0);
        }
    };
    auto sstore = [&](int buf) {
        float *as = lds + buf * (BM + BN) * LDS_LD, *bs = as + BM * LDS_LD;
#pragma unroll
        for (int j = 0; j < A_LD4; ++j) *reinterpret_cast<float4 *>(as + (lrow + 32 * j) * LDS_LD + lk) = ra[j];
#pragma unroll
        for (int j = 0; j < W_LD4; ++j) *reinterpret_cast<float4 *>(bs + (lrow + 32 * j) * LDS_LD + lk) = rw[j];
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

    if (ntiles > 0) {
        gload(0);
        sstore(0);
    }
    __syncthreads();

    const int li = lane & 31, lh = lane >> 5;
    for (int t = 0; t < ntiles; ++t) {
        const int buf = t & 1;
        if (t + 1 < ntiles) gload(t + 1);
        const float *as = lds + buf * (BM + BN) * LDS_LD + (wm * 32 * TM + li) * LDS_LD + 4 * lh;
        const float *bs = lds + buf * (BM + BN) * LDS_LD + BM * LDS_LD + (wn * 32 * TN + li) * LDS_LD + 4 * lh;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            float4 fa[TM], fb[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) fa[i] = *reinterpret_cast<const float4 *>(as + i * 32 * LDS_LD + 8 * c);
#pragma unroll
            for (int j = 0; j < TN; ++j) fb[j] = *reinterpret_cast<const float4 *>(bs + j * 32 * LDS_LD + 8 * c);
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i].x, fb[j].x, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i].y, fb[j].y, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i].z, fb[j].z, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i].w, fb[j].w, acc[i][j], 0, 0, 0);
                }
        }
        if (t + 1 < ntiles) sstore(buf ^ 1);
        __syncthreads();
    }

    if (g.ksplit > 1) {
        // raw partial sums straight from the D layout: row = (r&3) + 8*(r>>2) + 4*(lane>>5), col = lane&31
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int col = n0 + wn * 32 * TN + j * 32 + li;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = m0 + wm * 32 * TM + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                    if (row < g.M && col < g.N) g.ws[((size_t)bid.z * g.M + row) * g.N + col] = acc[i][j][r];
                }
            }
        return;
    }
    if constexpr (BM == 128) {
        // two 64-row halves: the statistics slabs are 64 rows for every tile shape (see the bf16x3 kernel)
        for (int half = 0; half < 2; ++half) {
            if (m0 + 64 * half >= g.M) break;   // uniform: no second slab behind the last valid row
            if (wm == half) {
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int rl = i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                            lds[rl * TLD + wn * 32 * TN + j * 32 + li] = acc[i][j][r];
                        }
            }
            __syncthreads();
            rowwise_epilogue<64, BN, false>(g, lds, TLD, m0 + 64 * half, n0, 2 * bid.y + half, lds);
            __syncthreads();
        }
        return;
    }
    // accumulators -> row-major LDS tile (the operand buffers are dead: the loop ended on a barrier)
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int rl = wm * 32 * TM + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                lds[rl * TLD + wn * 32 * TN + j * 32 + li] = acc[i][j][r];
            }
    __syncthreads();
    rowwise_epilogue<BM, BN, false>(g, lds, TLD, m0, n0, bid.y, lds);  // `red` aliases the tile: it is written after a barrier
}

// ------------------------------------------------------------------------------------------------------
// bf16x3 variant: every fp32 operand x is split on the fly into hi = bf16(x), lo = bf16(x - hi) and the product
// is formed as hi*hi + hi*lo + lo*hi on v_mfma_f32_32x32x16_bf16 with fp32 accumulation: ~2^-16 relative
// error per product (the dropped lo*lo term) at 16/3 = 5.3x the fp32 MFMA rate.  Same tiling, staging map,
// split-K and epilogue as the fp32 kernel; LDS holds a hi and a lo plane per operand, rows of BK3 bf16 padded
// by 16 B (conflict-free 16-B fragment reads).  Selected with COFI_GEMM_BF16X3 in `act`; static operands (weights) may arrive
// pre-split (COFI_GEMM_W_SPLIT, cofi_split_bf16_planes).
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ unsigned cvt_pk_bf16(float a, float b) {  // RNE, a -> low half
    unsigned r;
    asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ void split4(const f32x4 v, uint2 &hi, uint2 &lo) {
    hi.x = cvt_pk_bf16(v[0], v[1]);
    hi.y = cvt_pk_bf16(v[2], v[3]);
    const float rx = v[0] - __uint_as_float(hi.x << 16), ry = v[1] - __uint_as_float(hi.x & 0xffff0000u);
    const float rz = v[2] - __uint_as_float(hi.y << 16), rw = v[3] - __uint_as_float(hi.y & 0xffff0000u);
    lo.x = cvt_pk_bf16(rx, ry);
    lo.y = cvt_pk_bf16(rz, rw);
}
// three planes: hi + mid + lo carry all 24 mantissa bits of an fp32 value (the bf16x6 arithmetic)
__device__ __forceinline__ void split4x3(const f32x4 v, uint2 &hi, uint2 &mid, uint2 &lo) {
    hi.x = cvt_pk_bf16(v[0], v[1]);
    hi.y = cvt_pk_bf16(v[2], v[3]);
    const float rx = v[0] - __uint_as_float(hi.x << 16), ry = v[1] - __uint_as_float(hi.x & 0xffff0000u);
    const float rz = v[2] - __uint_as_float(hi.y << 16), rw = v[3] - __uint_as_float(hi.y & 0xffff0000u);
    mid.x = cvt_pk_bf16(rx, ry);
    mid.y = cvt_pk_bf16(rz, rw);
    lo.x = cvt_pk_bf16(rx - __uint_as_float(mid.x << 16), ry - __uint_as_float(mid.x & 0xffff0000u));
    lo.y = cvt_pk_bf16(rz - __uint_as_float(mid.y << 16), rw - __uint_as_float(mid.y & 0xffff0000u));
}
__device__ __forceinline__ void split4(const float4 v, uint2 &hi, uint2 &lo) {
    hi.x = cvt_pk_bf16(v.x, v.y);
    hi.y = cvt_pk_bf16(v.z, v.w);
    const float rx = v.x - __uint_as_float(hi.x << 16), ry = v.y - __uint_as_float(hi.x & 0xffff0000u);
    const float rz = v.z - __uint_as_float(hi.y << 16), rw = v.w - __uint_as_float(hi.y & 0xffff0000u);
    lo.x = cvt_pk_bf16(rx, ry);
    lo.y = cvt_pk_bf16(rz, rw);
}

// Static operands (weights) are split once: planes (2, N, ldp) bf16 = [hi | lo], rows zero-padded to ldp (multiple of 8).
// Same rounding as split4, so a pre-split launch is bit-identical to splitting on the fly.
__global__ void split_planes_kernel(const float *W, int ldw, int N, int K, unsigned *planes, int ldp, int nplanes) {
    const int hp = ldp >> 1;   // bf16 pairs per row
    const size_t total = (size_t)N * hp;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int n = (int)(i / hp), k = 2 * (int)(i - (size_t)n * hp);
        const float a = k < K ? W[(size_t)n * ldw + k] : 0.f, b = k + 1 < K ? W[(size_t)n * ldw + k + 1] : 0.f;
        const unsigned hi = cvt_pk_bf16(a, b);
        const float ra = a - __uint_as_float(hi << 16), rb = b - __uint_as_float(hi & 0xffff0000u);
        const unsigned lo = cvt_pk_bf16(ra, rb);   // two planes: lo; three planes: mid
        planes[i] = hi;
        planes[total + i] = lo;
        if (nplanes == 3) planes[2 * total + i] = cvt_pk_bf16(ra - __uint_as_float(lo << 16), rb - __uint_as_float(lo & 0xffff0000u));
    }
}

// K-tile of 128 per iteration (BK3): at batch 1 most problems give <= 1 workgroup per CU, so the loop is bound by
// the L2/HBM round trip per k-tile, not by the matrix cores; a 4x deeper tile keeps 4x the bytes in flight per wave
// and needs 4x fewer barriers.  One LDS buffer + a register-staged next tile:
//   issue global loads (t+1) -> MFMAs on tile t from LDS -> barrier -> split + write tile t+1 -> barrier.
// (The 128x128 tile uses BK3 = 64: 128 would need 139 KB of LDS and the whole VGPR file for one workgroup.)
// 4 waves (2x2 over the tile), up to 2-3 workgroups per CU.  (An 8 / 16-wave variant that split every K-tile over wave groups shortened a
// LONE launch but cost throughput with frames in flight - 563 vs 583 frames/s - and was removed in round 3)
// ANORM: the A operand carries a pending GroupNorm / InstanceNorm (+ affine + LeakyReLU) of the producing layer (GemmArgs::an):
//        the workgroup folds the producer's statistics partials itself while its first tile is in flight, keeps the per-channel
//        scale / shift in LDS and normalises every A element on its way into the bf16 planes - the stand-alone normalisation
//        kernel, its statistics kernel and one round trip of the activation through HBM disappear.
// ASPLIT: the A operand arrives PRE-SPLIT as well (bf16 hi / lo planes written by its producer - the KPConv aggregation, whose
//        (M, 15 C) output has no other reader): A tiles then travel global -> LDS as plain 16-byte copies like the W tiles, the
//        conversion instructions (the bulk of the VALU work of a tile) and their registers disappear.  Dense GEMM only.
//        (An earlier experiment in this slot - two K-tiles in flight in registers - measured 445 vs 457 frames/s and was removed.)
// X6 (COFI_GEMM_BF16X6): THREE bf16 planes per operand - hi + mid + lo hold all 24 mantissa bits of an fp32 value - and the six
//        products hi*hi + hi*mid + mid*hi + mid*mid + hi*lo + lo*hi (what is dropped is below 2^-24 of |a||b|): fp32-grade results
//        (the error is that of the fp32 accumulation, as in the exact-fp32 kernel) at 16/6 = 2.7x the fp32 MFMA rate.  Operands are
//        split on the fly (no pre-split planes); the normalising loader (ANORM) works as in the 3-term kernel.
template <int BM, int BN, int TM, int TN, int BK3, bool WSPLIT = false, int WPE = 1, bool ANORM = false, bool ASPLIT = false, bool X6 = false>
__global__ __launch_bounds__(256, WPE) void gemm_bf16x3_kernel(GemmArgs g) {
    static_assert(BM == 64 * TM && BN == 64 * TN, "2x2 waves");
    static_assert(!X6 || !ASPLIT, "bf16x6: A is split on the fly (W may arrive as three pre-split planes)");
    constexpr int NPL = X6 ? 3 : 2;   // bf16 planes per operand
    constexpr int NT = 256;
    // bytes per LDS row.  64- / 128-deep K-tiles: bf16 values + 16 B pad (36 / 68 dwords: conflict-free b128 reads, and a 16-lane group of
    // the b64 plane stores covers one row).  32-deep K-tiles (the wide bf16x6 tiles): that padding (20 dwords) lets two rows of a store group
    // overlap mod 32 banks - a third of the LDS cycles of the 128 x 128 bf16x6 kernel were bank conflicts (PMC, round 4) - so the rows stay
    // UNPADDED (64 B) and the four 16-byte chunks of row r are XOR-swizzled by (r >> 2) & 3: the 16 rows a b128 read group touches
    // ({0-3, 12-15, 20-27} and its shifts) land on 16 distinct 4-bank groups, a store group writes two whole rows = all 32 banks once.
    constexpr bool SWZ = BK3 == 32;
    constexpr int BROW3 = SWZ ? 64 : BK3 * 2 + 16;
    auto loff = [](int row, int kbyte) -> int {   // byte offset of (row, byte kbyte of the row's K-slice) inside a plane
        if constexpr (SWZ) return row * 64 + ((((kbyte >> 4) ^ (row >> 2)) & 3) << 4) + (kbyte & 15);
        else return row * BROW3 + kbyte;
    };
    constexpr int LPR = BK3 / 4;          // lanes per row slice (float4 each)
    constexpr int RPP = NT / LPR;         // rows per staging pass
    constexpr int A_LD4 = BM / RPP, W_LD4 = BN / RPP;            // float4 loads per thread and tile
    static_assert(A_LD4 >= 1 && W_LD4 >= 1, "tile too small for 256 threads");
    // pre-split W: 16-B chunks of 8 bf16; chunk c of a plane tile = (row c / CPR, k 8 * (c % CPR))
    constexpr int CPR = BK3 / 8, W_CH = BN * CPR / NT, A_CH = BM * CPR / NT;
    static_assert(!ASPLIT || ((BM * CPR) % NT == 0 && WSPLIT && !ANORM), "pre-split A: plane tile must divide over the threads");
    static_assert(!WSPLIT || (BN * CPR) % NT == 0, "plane tile must divide over the threads");
    constexpr int TLD = BN + 4;
    constexpr int PLANE_A = BM * BROW3, PLANE_W = BN * BROW3;    // bytes
    constexpr int BUF = NPL * (PLANE_A + PLANE_W);               // hi + lo (+ mid) of A and W
    // the epilogue re-uses the operand buffer as a row-major fp32 tile
    constexpr int EPI = (BM == 128 ? 64 : BM) * TLD * 4;   // BM = 128: two 64-row halves
    constexpr int LDS_BYTES = BUF > EPI ? BUF : EPI;
    static_assert((NT / (BN / 4)) * BN * 2 * 4 <= LDS_BYTES, "column-statistics scratch must fit");
    constexpr int AN_MAXC = 512;                                 // channels of a normalised A operand (scale + shift table behind the buffers)
    static_assert(!ANORM || (NT * 32 + AN_MAXC * 8 <= LDS_BYTES), "statistics fold scratch must fit in the operand buffer");
    __shared__ __attribute__((aligned(16))) unsigned char lds_raw[LDS_BYTES + (ANORM ? AN_MAXC * 8 : 0)];
    float *nsc = reinterpret_cast<float *>(lds_raw + LDS_BYTES), *nsh = nsc + AN_MAXC;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;   // position in the 2x2 wave grid
    const BlockId bid = gemm_block_id(g);
    const int m0 = bid.y * BM, n0 = bid.x * BN;
    const int kbeg = bid.z * g.kchunk;
    const int kend = min(g.K, kbeg + g.kchunk);
    const int ntiles = (kend - kbeg + BK3 - 1) / BK3;
    const int lrow = tid / LPR, lk = (tid % LPR) * 4;            // LPR lanes cover one row slice; RPP rows per pass
    struct Stage {                                               // one K-tile on its way from global memory to LDS
        f32x4 ra[ASPLIT ? 1 : A_LD4];                            // fp32 A: native vectors, plain 16-B loads, no struct copies
        f32x4 rah[ASPLIT ? A_CH : 1], ral[ASPLIT ? A_CH : 1];   // pre-split A: 16-B chunks (8 bf16) of the hi / lo plane
        f32x4 rw[WSPLIT ? 1 : W_LD4];                            // fp32 W: W_LD4 chunks of 4
        f32x4 rwh[WSPLIT ? W_CH : 1], rwl[WSPLIT ? W_CH : 1];   // pre-split W: 16-B chunks (8 bf16) of the hi / lo plane, as opaque bits
        f32x4 rwm[(WSPLIT && X6) ? W_CH : 1];                    // ... and of the mid plane (bf16x6: planes hi | mid | lo)
        unsigned amask;                                          // validity of the A values (see gload)
        bool afull;                                              // uniform: the A registers hold a full dense tile (no zeroing needed)
        int achan;                                               // ANORM: first of the 4 channels the staged float4s of this thread belong to
    };
    Stage st0;
    const bool conv = g.cv_ks != 0;

    // Addressing: a workgroup-uniform base (scalar registers, advanced by one K-tile per iteration) plus a per-thread 32-bit
    // byte offset that never changes -> the loads of a full tile need NO vector arithmetic at all.  Rows past M / N are
    // clamped to the last row: they only feed output rows / columns that are never stored (MFMA rows and columns are
    // independent), so they need no zeroing; only K tails (and convolution padding) are zeroed, on the A side.
    unsigned aoff[ASPLIT ? A_CH : A_LD4], woff[WSPLIT ? W_CH : W_LD4];
    if constexpr (ASPLIT) {
#pragma unroll
        for (int j = 0; j < A_CH; ++j) {
            const int c = tid + NT * j;
            aoff[j] = ((unsigned)(min(m0 + c / CPR, g.M - 1) - m0) * (unsigned)g.lda + 8 * (c % CPR)) * 2u;
        }
    } else {
#pragma unroll
        for (int j = 0; j < A_LD4; ++j) aoff[j] = ((unsigned)(min(m0 + lrow + RPP * j, g.M - 1) - m0) * (unsigned)g.lda + lk) * 4u;
    }
    if constexpr (WSPLIT) {
#pragma unroll
        for (int j = 0; j < W_CH; ++j) {
            const int c = tid + NT * j;
            woff[j] = ((unsigned)(min(n0 + c / CPR, g.N - 1) - n0) * (unsigned)g.ldw + 8 * (c % CPR)) * 2u;
        }
    } else {
#pragma unroll
        for (int j = 0; j < W_LD4; ++j) woff[j] = ((unsigned)(min(n0 + lrow + RPP * j, g.N - 1) - n0) * (unsigned)g.ldw + lk) * 4u;
    }
    const char *abase = ASPLIT ? reinterpret_cast<const char *>(reinterpret_cast<const uint16_t *>(g.A) + (size_t)m0 * g.lda + kbeg)
                               : reinterpret_cast<const char *>(g.A + (size_t)m0 * g.lda + kbeg);
    const size_t alo = (size_t)g.a_lo_off * 2;
    const char *wbase = WSPLIT ? reinterpret_cast<const char *>(reinterpret_cast<const uint16_t *>(g.W) + (size_t)n0 * g.ldw + kbeg)
                               : reinterpret_cast<const char *>(g.W + (size_t)n0 * g.ldw + kbeg);
    const size_t wlo = (size_t)g.w_lo_off * 2;

    // conv-mode pixel coordinates of this thread's A rows (row = m0 + lrow + RPP*j)
    int yo[A_LD4], xo[A_LD4], fb[A_LD4];
    if (!ASPLIT && conv) {
#pragma unroll
        for (int j = 0; j < A_LD4; ++j) {
            const int r = min(m0 + lrow + RPP * j, g.M - 1);
            const int f = r / g.cv_Pout, pix = r - f * g.cv_Pout;
            fb[j] = f * g.cv_H * g.cv_W;
            yo[j] = pix / g.cv_Wo;
            xo[j] = pix - yo[j] * g.cv_Wo;
        }
    }
    // Validity of the A values is kept as a bit mask and applied when the registers are consumed (sstore), so nothing touches
    // a loaded value - and no s_waitcnt is needed - until after the MFMAs.  Full dense tiles carry no mask at all.
    auto gload = [&](int t, Stage &st) {
        const bool full = kbeg + (t + 1) * BK3 <= kend;   // uniform
        const int k = kbeg + t * BK3 + lk;
        const bool kin = k < kend;
        if constexpr (ASPLIT) {
            const char *at = abase + (size_t)t * (BK3 * 2);
            const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
            if (full) {
#pragma unroll
                for (int j = 0; j < A_CH; ++j) {
                    st.rah[j] = *reinterpret_cast<const f32x4 *>(at + aoff[j]);
                    st.ral[j] = *reinterpret_cast<const f32x4 *>(at + alo + aoff[j]);
                }
            } else {   // K tail: chunks past the K range are ZERO (the W side re-reads finite values there); K is a multiple of 8
#pragma unroll
                for (int j = 0; j < A_CH; ++j) {
                    const int c8 = 8 * ((tid + NT * j) % CPR);
                    const bool cin = kbeg + t * BK3 + c8 < kend;
                    const char *q = cin ? at + aoff[j] : abase + (aoff[j] - 2u * c8);
                    const f32x4 h = *reinterpret_cast<const f32x4 *>(q), l = *reinterpret_cast<const f32x4 *>(q + alo);
                    st.rah[j] = cin ? h : zero;
                    st.ral[j] = cin ? l : zero;
                }
            }
        } else if (!conv) {
            if constexpr (ANORM) st.achan = kin ? k : 0;
            st.afull = full;
            const char *at = abase + (size_t)t * (BK3 * 4);
            if (full) {
#pragma unroll
                for (int j = 0; j < A_LD4; ++j) st.ra[j] = *reinterpret_cast<const f32x4 *>(at + aoff[j]);
            } else {
                st.amask = kin ? ~0u : 0u;   // lanes past the K range re-read the first values of their row (always in range)
#pragma unroll
                for (int j = 0; j < A_LD4; ++j) st.ra[j] = *reinterpret_cast<const f32x4 *>(kin ? at + aoff[j] : abase + (aoff[j] - 4u * lk));
            }
        } else {
            st.afull = false;
            const int kc = kin ? k : 0;
            const int tap = kc / g.cv_Cin, c = kc - tap * g.cv_Cin;
            const int dy = tap / g.cv_ks, dx = tap - dy * g.cv_ks;
            if constexpr (ANORM) st.achan = c;
            st.amask = 0;
#pragma unroll
            for (int j = 0; j < A_LD4; ++j) {
                const int yi = yo[j] * g.cv_stride - g.cv_pad + dy, xi = xo[j] * g.cv_stride - g.cv_pad + dx;
                const bool ok = kin && (unsigned)yi < (unsigned)g.cv_H && (unsigned)xi < (unsigned)g.cv_W;
                const int yc = min(max(yi, 0), g.cv_H - 1), xc = min(max(xi, 0), g.cv_W - 1);
                st.ra[j] = *reinterpret_cast<const f32x4 *>(g.A + ((size_t)fb[j] + (size_t)yc * g.cv_W + xc) * g.lda + c);
                st.amask |= ok ? (1u << j) : 0u;
            }
        }
        // W: lanes past the K range re-read the start of their row (finite values x zeroed A = 0)
        if constexpr (WSPLIT) {
            const char *wt = wbase + (size_t)t * (BK3 * 2);
            if (full) {
#pragma unroll
                for (int j = 0; j < W_CH; ++j) {
                    st.rwh[j] = *reinterpret_cast<const f32x4 *>(wt + woff[j]);
                    st.rwl[j] = *reinterpret_cast<const f32x4 *>(wt + (NPL - 1) * wlo + woff[j]);
                    if constexpr (X6) st.rwm[j] = *reinterpret_cast<const f32x4 *>(wt + wlo + woff[j]);
                }
            } else {  // chunks that start past the K range re-read the first chunk of their row (plane rows are padded to 8 values)
#pragma unroll
                for (int j = 0; j < W_CH; ++j) {
                    const int c8 = 8 * ((tid + NT * j) % CPR);
                    const bool cin = kbeg + t * BK3 + c8 < kend;
                    const char *q = cin ? wt + woff[j] : wbase + (woff[j] - 2u * c8);
                    st.rwh[j] = *reinterpret_cast<const f32x4 *>(q);
                    st.rwl[j] = *reinterpret_cast<const f32x4 *>(q + (NPL - 1) * wlo);
                    if constexpr (X6) st.rwm[j] = *reinterpret_cast<const f32x4 *>(q + wlo);
                }
            }
        } else {
            const char *wt = wbase + (size_t)t * (BK3 * 4);
            if (full) {
#pragma unroll
                for (int j = 0; j < W_LD4; ++j) st.rw[j] = *reinterpret_cast<const f32x4 *>(wt + woff[j]);
            } else {
#pragma unroll
                for (int j = 0; j < W_LD4; ++j) st.rw[j] = *reinterpret_cast<const f32x4 *>(kin ? wt + woff[j] : wbase + (woff[j] - 4u * lk));
            }
        }
    };
    auto sstore = [&](Stage &st) {
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
        if constexpr (ANORM) {
            // the pending normalisation of the producer: y * sc + sh, LeakyReLU as max(v, v * slope) (0 <= slope <= 1) - the
            // same operations in the same order as the stand-alone apply kernel.  Zero padding / K tails are masked afterwards.
            const f32x4 sc = *reinterpret_cast<const f32x4 *>(nsc + st.achan), sh = *reinterpret_cast<const f32x4 *>(nsh + st.achan);
#pragma unroll
            for (int j = 0; j < A_LD4; ++j) {
                f32x4 v = st.ra[j] * sc + sh;
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = v[e] >= 0.f ? v[e] : v[e] * g.an.slope;
                st.ra[j] = v;
            }
        }
        if constexpr (ASPLIT) {
#pragma unroll
            for (int j = 0; j < A_CH; ++j) {
                const int c = tid + NT * j;
                unsigned char *p = lds_raw + loff(c / CPR, (c % CPR) * 16);
                *reinterpret_cast<f32x4 *>(p) = st.rah[j];
                *reinterpret_cast<f32x4 *>(p + PLANE_A) = st.ral[j];
            }
        } else {
#pragma unroll
            for (int j = 0; j < A_LD4; ++j) {
                const f32x4 v = (st.afull || ((st.amask >> j) & 1u)) ? st.ra[j] : zero;
                unsigned char *p = lds_raw + loff(lrow + RPP * j, lk * 2);
                uint2 hi, lo;
                if constexpr (X6) {   // planes: hi | mid | lo
                    uint2 mid;
                    split4x3(v, hi, mid, lo);
                    *reinterpret_cast<uint2 *>(p + PLANE_A) = mid;
                    *reinterpret_cast<uint2 *>(p + 2 * PLANE_A) = lo;
                } else {
                    split4(v, hi, lo);
                    *reinterpret_cast<uint2 *>(p + PLANE_A) = lo;
                }
                *reinterpret_cast<uint2 *>(p) = hi;
            }
        }
        if constexpr (WSPLIT) {
#pragma unroll
            for (int j = 0; j < W_CH; ++j) {
                const int c = tid + NT * j;
                unsigned char *p = lds_raw + NPL * PLANE_A + loff(c / CPR, (c % CPR) * 16);
                *reinterpret_cast<f32x4 *>(p) = st.rwh[j];
                *reinterpret_cast<f32x4 *>(p + (NPL - 1) * PLANE_W) = st.rwl[j];
                if constexpr (X6) *reinterpret_cast<f32x4 *>(p + PLANE_W) = st.rwm[j];
            }
        } else {
#pragma unroll
            for (int j = 0; j < W_LD4; ++j) {
                uint2 hi, lo;
                unsigned char *p = lds_raw + NPL * PLANE_A + loff(lrow + RPP * j, lk * 2);
                if constexpr (X6) {
                    uint2 mid;
                    split4x3(st.rw[j], hi, mid, lo);
                    *reinterpret_cast<uint2 *>(p + PLANE_W) = mid;
                    *reinterpret_cast<uint2 *>(p + 2 * PLANE_W) = lo;
                } else {
                    split4(st.rw[j], hi, lo);
                    *reinterpret_cast<uint2 *>(p + PLANE_W) = lo;
                }
                *reinterpret_cast<uint2 *>(p) = hi;
            }
        }
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

    const int li = lane & 31, lh = lane >> 5;
    union Frag { uint4 u; bf16x8 v; };
    constexpr int STEPS = BK3 / 16;   // 16-deep MFMA steps per tile
    // lane (li, lh) reads chunk 2 s2 + lh of its row; every row this lane touches is li mod 32, so the swizzle term is a lane constant
    const unsigned char *as = lds_raw + (wm * 32 * TM + li) * BROW3 + (SWZ ? 0 : lh * 16);
    const unsigned char *bs = lds_raw + NPL * PLANE_A + (wn * 32 * TN + li) * BROW3 + (SWZ ? 0 : lh * 16);
    const int swz = (li >> 2) & 3;
    auto koff = [&](int s2) -> int { return SWZ ? (((2 * s2 + lh) ^ swz) << 4) : s2 * 32; };
    auto compute = [&]() {
#pragma unroll
        for (int s2 = 0; s2 < STEPS; ++s2) {  // lane (i,h) owns k = 16*s2 + 8h .. +7
            Frag ah[TM], al[TM], bh[TN], bl[TN], am[X6 ? TM : 1], bm[X6 ? TN : 1];
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                ah[i].u = *reinterpret_cast<const uint4 *>(as + i * 32 * BROW3 + koff(s2));
                al[i].u = *reinterpret_cast<const uint4 *>(as + (NPL - 1) * PLANE_A + i * 32 * BROW3 + koff(s2));
                if constexpr (X6) am[i].u = *reinterpret_cast<const uint4 *>(as + PLANE_A + i * 32 * BROW3 + koff(s2));
            }
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                bh[j].u = *reinterpret_cast<const uint4 *>(bs + j * 32 * BROW3 + koff(s2));
                bl[j].u = *reinterpret_cast<const uint4 *>(bs + (NPL - 1) * PLANE_W + j * 32 * BROW3 + koff(s2));
                if constexpr (X6) bm[j].u = *reinterpret_cast<const uint4 *>(bs + PLANE_W + j * 32 * BROW3 + koff(s2));
            }
            // product-major order: consecutive MFMAs go to DIFFERENT accumulator tiles (TM x TN independent chains), so none waits for
            // the result of the one issued right before it; per accumulator the order of the terms is unchanged (smallest first)
            auto term = [&](auto pa, auto pb) {
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pa(i), pb(j), acc[i][j], 0, 0, 0);
            };
            auto AH = [&](int i) { return ah[i].v; };
            auto AL = [&](int i) { return al[i].v; };
            auto BH = [&](int j) { return bh[j].v; };
            auto BL = [&](int j) { return bl[j].v; };
            if constexpr (X6) {   // smallest terms first: 2^-16 (lo*hi, hi*lo, mid*mid), 2^-8 (mid*hi, hi*mid), 1 (hi*hi)
                auto AM = [&](int i) { return am[i].v; };
                auto BM_ = [&](int j) { return bm[j].v; };
                term(AL, BH);
                term(AH, BL);
                term(AM, BM_);
                term(AM, BH);
                term(AH, BM_);
                term(AH, BH);
            } else {
                term(AL, BH);
                term(AH, BL);
                term(AH, BH);
            }
        }
    };
    // One LDS buffer + a register-staged next tile: issue global loads (t+1) -> MFMAs on tile t -> barrier -> split + write
    // tile t+1 -> barrier.  (Measured on MI355X: deeper register prefetch (2-3 tiles in flight, exact vmcnt) and a second LDS
    // buffer do NOT shorten the ~1 us a lone workgroup spends per 64 KB tile - that is the CU's L2 fill rate; only spreading
    // the tiles over more CUs does, which is what split-K is tuned for.)
    if (ntiles > 0) gload(0, st0);
    if constexpr (ANORM) {
        // statistics of this tile's frame -> scale / shift table in LDS: copied from the finalized vectors (cofi_norm_finalize) or,
        // without them, folded here from the producer's partials (fold scratch lives in the still unused operand buffer)
        const int f = g.an_rows > 0 ? m0 / g.an_rows : 0;
        if (g.an.scsh) {
            const float *src = g.an.scsh + (size_t)f * 2 * g.an.C;
            for (int c = tid * 4; c < g.an.C; c += NT * 4) {
                *reinterpret_cast<f32x4 *>(nsc + c) = *reinterpret_cast<const f32x4 *>(src + c);
                *reinterpret_cast<f32x4 *>(nsh + c) = *reinterpret_cast<const f32x4 *>(src + g.an.C + c);
            }
        } else {
            double *dred = reinterpret_cast<double *>(lds_raw);
            float *sstat = reinterpret_cast<float *>(lds_raw + NT * 32);
            fold_stat_table<NT, 6>(g.an.part + (size_t)f * g.an.nslab * g.an.tcols * 2, g.an.nslab, g.an.tcols, g.an.groups, g.an.count, g.an.eps,
                                   dred, sstat);
            norm_scale_shift<NT>(g.an, sstat, nsc, nsh);
        }
        __syncthreads();
    }
    if (ntiles > 0) sstore(st0);
    __syncthreads();
    {
        for (int t = 0; t < ntiles; ++t) {
            if (t + 1 < ntiles) gload(t + 1, st0);
            compute();
            __syncthreads();              // every wave is done reading tile t
            if (t + 1 < ntiles) {
                sstore(st0);
                __syncthreads();          // tile t+1 visible
            }
        }
    }

    float *lds = reinterpret_cast<float *>(lds_raw);
    if (g.ksplit > 1) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int col = n0 + wn * 32 * TN + j * 32 + li;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = m0 + wm * 32 * TM + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                    if (row < g.M && col < g.N) g.ws[((size_t)bid.z * g.M + row) * g.N + col] = acc[i][j][r];
                }
            }
        return;
    }
    if constexpr (BM == 128) {
        // epilogue in two 64-row halves (statistics slabs of 64 rows): half the LDS tile, so the operand buffer - not the epilogue -
        // sizes the workgroup's LDS and a third workgroup fits on the CU
        for (int half = 0; half < 2; ++half) {
            if (m0 + 64 * half >= g.M) break;   // uniform: a last tile with <= 64 valid rows has no second slab (its table entry does not exist)
            if (wm == half) {
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int rl = i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                            lds[rl * TLD + wn * 32 * TN + j * 32 + li] = acc[i][j][r];
                        }
            }
            __syncthreads();
            rowwise_epilogue<64, BN, false>(g, lds, TLD, m0 + 64 * half, n0, 2 * bid.y + half, lds);
            __syncthreads();
        }
        return;
    }
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int rl = wm * 32 * TM + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                lds[rl * TLD + wn * 32 * TN + j * 32 + li] = acc[i][j][r];
            }
    __syncthreads();
    rowwise_epilogue<BM, BN, false>(g, lds, TLD, m0, n0, bid.y, lds);
}

#include "gemm_planes.inc"
#include "gemm_x6_big.inc"
#include "gemm_f16_big.inc"
#include "conv_direct.inc"

// split-K tail, same row-wise epilogue reading the partial sums.  Two tilings:
//   64 rows x 32 columns  (plain / column statistics): slabs of 64 rows keep the statistics table small and
//                          even M = 1280, N = 256 still gives 160 workgroups;
//   16 rows x 128 columns (fused LayerNorm): a tile spans whole rows (N <= 128).
constexpr int SK_ROWS = 64, SK_COLS = 32, SKLN_ROWS = 16;
template <int COLS>   // 32; 64 when a statistics table entry spans 64 columns
__global__ __launch_bounds__(256) void splitk_epilogue_kernel(GemmArgs g) {
    __shared__ float red[(256 / (COLS / 4)) * COLS * 2];
    rowwise_epilogue<SK_ROWS, COLS, true>(g, nullptr, 0, blockIdx.y * SK_ROWS, blockIdx.x * COLS, blockIdx.y, red);
}
__global__ __launch_bounds__(256) void splitk_epilogue_ln_kernel(GemmArgs g) {
    rowwise_epilogue<SKLN_ROWS, 128, true>(g, nullptr, 0, blockIdx.y * SKLN_ROWS, blockIdx.x * 128, blockIdx.y, nullptr);
}

}  // namespace

// The host side from here on.  Which kernel, tile, K split and workspace layout a contraction gets is decided in gemm_planner.h alone
// (PlanRequest -> status + Plan); the entries below validate operands, ask it, fill GemmArgs from request and plan, and call launch().
#include "gemm_planner.h"

namespace {

static_assert(PLAN_BK == BK, "the planner's K-tile is the register-staged kernels'");

thread_local long g_f16_launches = 0;     // launches of the calling thread that took gemm_f16_big_kernel, and their 2 M N K (cofi_tune_f16x3_launch_flops)
thread_local double g_f16_flops = 0.0;

// Tile order (GemmArgs::xcd): estimate the bytes both orders pull over the fabric — every XCD that touches a row panel of A
// or a column panel of W reads it through its own L2 — and take the cheaper one.
int xcd_order(const GemmArgs &g, const dim3 &grid) {
    const int mode = 2;   // 0 / 1 would force hardware / XCD-contiguous order; 2 picks per launch from the traffic estimate below
    const long gx = grid.x, gy = grid.y, gz = grid.z, nblk = gx * gy * gz;
    if (mode == 0 || (gx & (gx - 1)) || nblk < 16 || gy * gz >= 65536) return 0;
    const int enc = 1 + __builtin_ctzl(gx);
    if (mode == 1) return enc;
    auto gcd = [](long a, long b) { while (b) { long t = a % b; a = b; b = t; } return a; };
    const double abytes = (double)g.M * g.K, wbytes = (double)g.N * g.K;
    // hardware order: workgroup L -> XCD L % 8, L = (z*gy + y)*gx + x
    const double rr = abytes * std::min(gx, 8L) + wbytes * std::min(gy, 8 / gcd(gx % 8 ? gx % 8 : 8, 8));
    // contiguous order: XCD c owns workgroups [c*nblk/8, (c+1)*nblk/8) -> a K-slice of W is shared by ceil(8/gz) XCDs
    const double a_rep = std::min(8.0, std::max(1.0, 8.0 * gx / nblk));
    const double ct = abytes * a_rep + wbytes * std::min(std::min(gy, 8L), (8 + gz - 1) / gz);
    return ct < rr ? enc : 0;
}

int launch_direct(const GemmArgs &g, const Plan &p, hipStream_t s);

int launch(const GemmArgs &g0, const Plan &p, hipStream_t s) {
    if (plan_is_direct(p)) return launch_direct(g0, p, s);
    GemmArgs g = g0;
    g.ksplit = p.ksplit;
    g.kchunk = p.kchunk;
    dim3 grid(cofi_cdiv(g.N, p.bn), cofi_cdiv(g.M, p.bm), p.ksplit);
    g.xcd = xcd_order(g, grid);
    g.dbg = g_big_dbg;
    g.xcd_rcp_gy = grid.y > 1 ? (unsigned)((0x100000000ULL + grid.y - 1) / grid.y) : 0u;   // 0: gy = 1
    if (p.family == COFI_PLAN_PLANES) {
        switch (p.pcfg) {
#define X(id, bm_, bn_, bk_, wm_, wn_, nst_, minw_)                                                                                      \
    case id:                                                                                                                             \
        hipLaunchKernelGGL((gemm_planes_kernel<bm_, bn_, bk_, wm_, wn_, nst_, minw_>), grid, dim3(64 * wm_ * wn_), 0, s, g);              \
        break;
            COFI_PLANES_CFGS(X)
#undef X
        default: return COFI_EINVAL;
        }
    } else if (p.big) {
        const bool cv = g.cv_ks != 0;
#define COFI_LAUNCH_BIG(BN_)                                                                                                  \
    do {                                                                                                                      \
        if (g.an.part && cv) hipLaunchKernelGGL((gemm_x6_big_kernel<true, true, BN_>), grid, dim3(256), 0, s, g);            \
        else if (g.an.part) hipLaunchKernelGGL((gemm_x6_big_kernel<true, false, BN_>), grid, dim3(256), 0, s, g);            \
        else if (cv) hipLaunchKernelGGL((gemm_x6_big_kernel<false, true, BN_>), grid, dim3(256), 0, s, g);                   \
        else hipLaunchKernelGGL((gemm_x6_big_kernel<false, false, BN_>), grid, dim3(256), 0, s, g);                          \
    } while (0)
        if (plan_is_f16x3(p)) {
            ++g_f16_launches;
            g_f16_flops += 2.0 * g.M * g.N * g.K;
            // the pipelined kernel, then the repair launch over the same grid (its workgroups exit at once unless the first one flagged their tile)
#define COFI_LAUNCH_F16B(ROBUST_, NW_, WPRE_, BM_)                                                                                                  \
    do {                                                                                                                                            \
        if (g.an.part && cv) hipLaunchKernelGGL((gemm_f16_big_kernel<true, true, ROBUST_, NW_, WPRE_, BM_>), grid, dim3(64 * NW_), 0, s, g);       \
        else if (g.an.part) hipLaunchKernelGGL((gemm_f16_big_kernel<true, false, ROBUST_, NW_, WPRE_, BM_>), grid, dim3(64 * NW_), 0, s, g);       \
        else if (cv) hipLaunchKernelGGL((gemm_f16_big_kernel<false, true, ROBUST_, NW_, WPRE_, BM_>), grid, dim3(64 * NW_), 0, s, g);              \
        else hipLaunchKernelGGL((gemm_f16_big_kernel<false, false, ROBUST_, NW_, WPRE_, BM_>), grid, dim3(64 * NW_), 0, s, g);                     \
    } while (0)
#define COFI_LAUNCH_F16(ROBUST_, NW_, WPRE_) COFI_LAUNCH_F16B(ROBUST_, NW_, WPRE_, 256)
            if (p.family == COFI_PLAN_BIG_F16_128) {   // pre-split W, 128 x 128 tiles: two workgroups per CU
                COFI_LAUNCH_F16B(false, 4, true, 128);
                COFI_LAUNCH_F16B(true, 4, true, 128);
            } else if (g.wscale) {      // pre-split W (eight-wave geometry only)
                COFI_LAUNCH_F16(false, 8, true);
                COFI_LAUNCH_F16(true, 8, true);
            } else if (p.family == COFI_PLAN_BIG_F16_W4) {   // cofi_tune_big_debug bit 256 (A/B): the four-wave geometry
                COFI_LAUNCH_F16(false, 4, false);
                COFI_LAUNCH_F16(true, 4, false);
            } else {
                COFI_LAUNCH_F16(false, 8, false);
                COFI_LAUNCH_F16(true, 8, false);
            }
#undef COFI_LAUNCH_F16
#undef COFI_LAUNCH_F16B
        } else {
            COFI_LAUNCH_BIG(128);
        }
#undef COFI_LAUNCH_BIG
    } else if (g.bf16x3 == 2) {
        // bf16x6: three planes per operand; K-tiles of 64 (64 x 64 tile: 54 KB of LDS) / 32 (wider tiles: 41 / 60 KB)
#define COFI_LAUNCH_BF16X6(BM_, BN_, TM_, TN_, BK_)                                                                        \
    do {                                                                                                                  \
        if (g.wsplit && g.an.part)                                                                                        \
            hipLaunchKernelGGL((gemm_bf16x3_kernel<BM_, BN_, TM_, TN_, BK_, true, 1, true, false, true>), grid, dim3(256), 0, s, g);    \
        else if (g.wsplit)                                                                                                \
            hipLaunchKernelGGL((gemm_bf16x3_kernel<BM_, BN_, TM_, TN_, BK_, true, 1, false, false, true>), grid, dim3(256), 0, s, g);   \
        else if (g.an.part)                                                                                               \
            hipLaunchKernelGGL((gemm_bf16x3_kernel<BM_, BN_, TM_, TN_, BK_, false, 1, true, false, true>), grid, dim3(256), 0, s, g);   \
        else                                                                                                              \
            hipLaunchKernelGGL((gemm_bf16x3_kernel<BM_, BN_, TM_, TN_, BK_, false, 1, false, false, true>), grid, dim3(256), 0, s, g);  \
    } while (0)
        if (p.bm == 128 && p.bn == 128)
            COFI_LAUNCH_BF16X6(128, 128, 2, 2, 32);
        else if (p.bm == 64 && p.bn == 128)
            COFI_LAUNCH_BF16X6(64, 128, 1, 2, 32);
        else if (p.bm == 128 && p.bn == 64)
            COFI_LAUNCH_BF16X6(128, 64, 2, 1, 32);
        else
            COFI_LAUNCH_BF16X6(64, 64, 1, 1, 64);
#undef COFI_LAUNCH_BF16X6
    } else if (g.bf16x3) {
#define COFI_LAUNCH_BF16X3(BM_, BN_, TM_, TN_, BK_)                                                                        \
    do {                                                                                                                  \
        if (g.an.part)                                                                                                    \
            hipLaunchKernelGGL((gemm_bf16x3_kernel<BM_, BN_, TM_, TN_, BK_, true, 1, true, false>), grid, dim3(256), 0, s, g);    \
        else if (g.asplit)                                                                                                \
            hipLaunchKernelGGL((gemm_bf16x3_kernel<BM_, BN_, TM_, TN_, BK_, true, 1, false, true>), grid, dim3(256), 0, s, g);    \
        else if (g.wsplit)                                                                                                \
            hipLaunchKernelGGL((gemm_bf16x3_kernel<BM_, BN_, TM_, TN_, BK_, true, 1, false, false>), grid, dim3(256), 0, s, g);   \
        else                                                                                                              \
            hipLaunchKernelGGL((gemm_bf16x3_kernel<BM_, BN_, TM_, TN_, BK_, false, 1, false, false>), grid, dim3(256), 0, s, g);  \
    } while (0)
        // K-tile depth 64 for every tile shape (measured: the 64x128 and 64x64 tiles run 1.4x / 1.05x faster with 64-deep K-tiles -
        // 2-3 workgroups per CU instead of 1-2 - than with 128-deep ones; the 128x128 tile is register-bound at 2 waves per SIMD either way)
        if (p.bm == 128 && p.bn == 128)
            COFI_LAUNCH_BF16X3(128, 128, 2, 2, 64);
        else if (p.bm == 64 && p.bn == 128)
            COFI_LAUNCH_BF16X3(64, 128, 1, 2, 64);
        else
            COFI_LAUNCH_BF16X3(64, 64, 1, 1, 64);
#undef COFI_LAUNCH_BF16X3
    } else if (p.bm == 128 && p.bn == 128)
        hipLaunchKernelGGL((gemm_kernel<128, 128, 2, 2>), grid, dim3(256), 0, s, g);
    else if (p.bm == 64 && p.bn == 128)
        hipLaunchKernelGGL((gemm_kernel<64, 128, 1, 2>), grid, dim3(256), 0, s, g);
    else
        hipLaunchKernelGGL((gemm_kernel<64, 64, 1, 1>), grid, dim3(256), 0, s, g);
    if (p.ksplit > 1) {
        if (g.ln_gamma || g.l2n)
            hipLaunchKernelGGL(splitk_epilogue_ln_kernel, dim3(1, cofi_cdiv(g.M, SKLN_ROWS)), dim3(256), 0, s, g);
        else if (g.colpart && g.stat_shift > 5)
            hipLaunchKernelGGL(splitk_epilogue_kernel<64>, dim3(cofi_cdiv(g.N, 64), cofi_cdiv(g.M, SK_ROWS)), dim3(256), 0, s, g);
        else
            hipLaunchKernelGGL(splitk_epilogue_kernel<SK_COLS>, dim3(cofi_cdiv(g.N, SK_COLS), cofi_cdiv(g.M, SK_ROWS)), dim3(256), 0, s, g);
    }
    return cofi_launch_status();
}

// the direct 3 x 3 convolution (conv_direct.inc): one workgroup per tile of th rows x 64 pixels of a frame
int launch_direct(const GemmArgs &g, const Plan &p, hipStream_t s) {
    const int th = p.family == COFI_PLAN_DIRECT_4 ? 4 : 2;
    const long tiles = (long)(g.M / g.cv_Pout) * (g.cv_H / th) * (g.cv_W / 64);
    const dim3 grid(g.N / 64, (unsigned)tiles);
    if (th == 4) {
        if (g.an.part) hipLaunchKernelGGL((conv3x3_direct_kernel<true, 4>), grid, dim3(256), 0, s, g);
        else hipLaunchKernelGGL((conv3x3_direct_kernel<false, 4>), grid, dim3(256), 0, s, g);
    } else {
        if (g.an.part) hipLaunchKernelGGL((conv3x3_direct_kernel<true, 2>), grid, dim3(256), 0, s, g);
        else hipLaunchKernelGGL((conv3x3_direct_kernel<false, 2>), grid, dim3(256), 0, s, g);
    }
    return cofi_launch_status();
}

int check_common(const float *A, int lda, const float *W, int ldw, float *C, int ldc, int M, int N, int K) {
    if (!A || !W || !C || M < 0 || N <= 0 || K <= 0) return COFI_EINVAL;
    if ((K & 3) || (lda & 3) || (ldw & 3) || lda < K || ldw < K || ldc < N) return COFI_EINVAL;
    if (((uintptr_t)A & 15) || ((uintptr_t)W & 15)) return COFI_EINVAL;
    return 0;
}

// log2 of the statistics table width, or -1 if it cannot be used with N columns
int stat_shift_of(int width, int N) {
    if (width <= 0 || width > 64 || (width & (width - 1)) || (N % width)) return -1;
    int sh = 0;
    while ((1 << sh) < width) ++sh;
    return sh;
}

// ---- requests, as the entries, the queries and the description hooks put them to the planner
PlanRequest gemm_request(int M, int N, int K, int act, int pending_norm, int frames, size_t ws_bytes) {
    PlanRequest r = decode_flags(act);
    r.M = M; r.N = N; r.K = K; r.pending_norm = pending_norm; r.frames = frames; r.ws_bytes = ws_bytes;
    return r;
}

// cofi_gemm_f32_layernorm reads the arithmetic and COFI_GEMM_W_SPLIT from its `relu` word; it never takes the 256 x 128 kernel
PlanRequest layernorm_request(int M, int N, int K, int relu, size_t ws_bytes) {
    PlanRequest r = gemm_request(M, N, K, relu, 0, 1, ws_bytes);
    r.asplit = r.l2n = r.f16 = r.wf16 = 0;
    r.fused_ln = 1;
    return r;
}

PlanRequest conv_request(int H, int W, int Cin, int Cout, int ks, int stride, int pad, int ldx, int act, int pending_norm, int frames, size_t ws_bytes) {
    PlanRequest r = gemm_request(0, 0, 0, act, pending_norm, frames, ws_bytes);
    r.H = H; r.W = W; r.Cin = Cin; r.Cout = Cout; r.ks = ks; r.stride = stride; r.pad = pad; r.ldx = ldx;
    return r;
}

// The pending normalisation of the A operand (channels = columns of a dense A / input channels of a convolution) into g.an; the status goes
// into the request, and the planner reports it at its place among the other refusals.
int norm_status(GemmArgs &g, const cofi_norm_desc_t *a_norm, int channels, int a_rows_per_frame, int frames) {
    if (a_norm->channels != channels) return COFI_EINVAL;
    if (int rc = make_norm_src(a_norm, a_rows_per_frame, frames, 512, &g.an)) return rc;
    if (!(g.an.slope >= 0.f && g.an.slope <= 1.f)) return COFI_EINVAL;
    return 0;
}

// the f16x3 kernels' operands: tile flags in the workspace where the plan put them, the panel scales of a pre-split W behind its (N, ldw) matrix
void set_f16_args(GemmArgs &g, const PlanRequest &rq, const Plan &p, void *ws, const float *W, int ldw) {
    if (p.flag_off >= 0) {
        g.f16 = 1;
        g.fixflags = reinterpret_cast<unsigned *>(static_cast<char *>(ws) + p.flag_off);
    }
    if (rq.wf16) g.wscale = W + (size_t)rq.N * ldw;
}

int gemm_entry(const float *A, int lda, const cofi_norm_desc_t *a_norm, const float *W, int ldw, float *C, int ldc, int M, int N, int K,
               const float *bias, const float *rowdiv, int act, float *colpart, int stat_width, void *ws, size_t ws_bytes, int frames,
               cofi_stream_t stream, const float *res = nullptr, int ldr = 0, const int32_t *res_idx = nullptr, int res_idx_stride = 0,
               int res_rows = 0) {
    if (int rc = check_common(A, lda, W, ldw, C, ldc, M, N, K)) return rc;
    if ((res_idx && !res) || (res && ldr < N)) return COFI_EINVAL;
    if (res_idx && (res_rows <= 0 || res_idx_stride <= 0 || frames <= 0 || M % frames)) return COFI_EINVAL;
    if (res_idx && (long)frames * res_rows > 0x7fffffffL) return COFI_EINVAL;   // res_src_row computes the source row as an int
    if (M == 0) return 0;
    PlanRequest rq = gemm_request(M, N, K, act, a_norm ? 1 : 0, frames, ws ? ws_bytes : 0);
    const int sshift = colpart ? stat_shift_of(stat_width, N) : 0;
    rq.operands_ok = sshift >= 0 && !(rq.wsplit && (ldw & 7)) && !(rq.asplit && (lda & 7));   // pre-split planes: rows of 8 values
    GemmArgs g{};
    if (a_norm && frames > 0) rq.norm_status = norm_status(g, a_norm, K, M / frames, frames);
    Plan p;
    if (int rc = plan_gemm(rq, p)) return rc;
    g.A = A; g.W = W; g.C = C; g.bias = bias; g.rowdiv = rowdiv; g.ws = (float *)ws; g.colpart = colpart;
    g.lda = lda; g.ldw = ldw; g.ldc = ldc; g.M = M; g.N = N; g.K = K; g.act = rq.act; g.ksplit = 1;
    g.bf16x3 = rq.arith; g.wsplit = rq.wsplit; g.w_lo_off = (long)N * ldw; g.cv_Pout = 1; g.stat_shift = sshift;
    g.asplit = rq.asplit; g.a_lo_off = (long)M * lda;
    g.l2n = rq.l2n;
    g.res = res; g.ldr = ldr;
    if (res_idx) { g.res_idx = res_idx; g.res_idx_stride = res_idx_stride; g.res_rows = res_rows; g.res_out_rows = M / frames; }
    if (a_norm) g.an_rows = M / frames;
    set_f16_args(g, rq, p, ws, W, ldw);
    return launch(g, p, cofi_s(stream));
}

int conv_entry(const float *x, int ldx, const cofi_norm_desc_t *x_norm, int H, int W, int Cin, const float *Wt, int Cout, int ks, int stride,
               int pad, const float *bias, const float *res, int ldr, int act, int act_col0, float *y, int ldy, float *colpart, int stat_width,
               void *ws, size_t ws_bytes, int frames, cofi_stream_t stream) {
    if (!x || !Wt || !y || act_col0 < 0 || act_col0 > Cout) return COFI_EINVAL;
    if ((Cin & 3) || (ldx & 3) || ldx < Cin || ldy < Cout || (res && ldr < Cout) || ((uintptr_t)x & 15) || ((uintptr_t)Wt & 15)) return COFI_EINVAL;
    PlanRequest rq = conv_request(H, W, Cin, Cout, ks, stride, pad, ldx, act, x_norm ? (x_norm->scale_shift ? 2 : 1) : 0, frames, ws ? ws_bytes : 0);
    const int sshift = colpart ? stat_shift_of(stat_width, Cout) : 0;
    rq.operands_ok = sshift >= 0;
    GemmArgs g{};
    if (x_norm && frames > 0) rq.norm_status = norm_status(g, x_norm, Cin, H * W, frames);   // statistics of the INPUT map: H * W rows per frame
    Plan p;
    if (int rc = plan_conv(rq, p)) return rc;
    const int M = rq.M, K = rq.K;
    const int ldw = rq.wsplit ? (K + 7) / 8 * 8 : K;   // pre-split planes: rows padded to 8 values
    g.A = x; g.W = Wt; g.C = y; g.bias = bias; g.ws = (float *)ws; g.colpart = colpart; g.res = res;
    g.lda = ldx; g.ldw = ldw; g.ldc = ldy; g.ldr = ldr; g.M = M; g.N = Cout; g.K = K; g.act = rq.act; g.ksplit = 1;
    g.bf16x3 = rq.arith; g.wsplit = rq.wsplit; g.w_lo_off = (long)Cout * ldw;
    g.cv_ks = ks; g.cv_H = H; g.cv_W = W; g.cv_Cin = Cin; g.cv_Wo = conv_out_size(W, rq); g.cv_stride = stride; g.cv_pad = pad; g.cv_Pout = M / frames;
    g.stat_shift = sshift;
    g.act_col0 = act_col0;
    g.l2n = rq.l2n;
    if (x_norm) g.an_rows = M / frames;
    set_f16_args(g, rq, p, ws, Wt, ldw);
    return launch(g, p, cofi_s(stream));
}

int describe(int rc, const Plan &p, cofi_plan_desc_t *out) {
    *out = cofi_plan_desc_t{};
    out->status = rc;
    if (rc) return rc;
    out->family = p.family;
    out->bm = p.bm; out->bn = p.bn; out->ksplit = p.ksplit; out->kchunk = p.kchunk; out->pcfg = p.pcfg;
    out->partial_bytes = (long long)p.partial_bytes;
    out->flag_offset = p.flag_off;
    out->ws_bytes = (long long)p.ws_bytes;
    return 0;
}

}  // namespace

// Would a COFI_GEMM_BF16X6 | COFI_GEMM_F16X3 launch of this shape run on gemm_f16_big_kernel (with a workspace of cofi_gemm_f32_workspace bytes)?
// The planner's answer for that request: a caller holding a pre-split W (COFI_GEMM_W_F16PRE) asks before it passes it.
extern "C" int cofi_gemm_f16x3_eligible(int M, int N, int K, int pending_norm, int frames) {
    if (M <= 0 || N <= 0 || K <= 0 || frames <= 0) return 0;
    Plan p;
    return plan_gemm(gemm_request(M, N, K, COFI_GEMM_BF16X6 | COFI_GEMM_F16X3, pending_norm ? 1 : 0, frames, cofi_gemm_f32_workspace(M, N, K)), p) == 0 &&
           plan_is_f16x3(p);
}

extern "C" int cofi_conv2d_f16x3_eligible(int H, int W, int Cin, int Cout, int ks, int stride, int pad, int ldx, int pending_norm, int frames) {
    PlanRequest r = conv_request(H, W, Cin, Cout, ks, stride, pad, ldx, COFI_GEMM_BF16X6 | COFI_GEMM_F16X3, pending_norm ? 1 : 0, frames, 0);
    if (!conv_contraction(r)) return 0;
    r.ws_bytes = cofi_gemm_f32_workspace(r.M, r.N, r.K);
    Plan p;
    return plan_conv(r, p) == 0 && plan_is_f16x3(p);
}

// The most any plan of (M, N, K) uses, over the operand forms a caller can pass: fp32 / bf16x3, both operands pre-split, bf16x6 with
// pre-split and with fp32 weights (the 256 x 128 kernel's shapes), f16x3 (its own table of shapes and splits, and its tile flags)
extern "C" size_t cofi_gemm_f32_workspace(int M, int N, int K) {
    if (M <= 0 || N <= 0 || K <= 0) return 0;
    size_t need = 0;
    for (const int form : {COFI_GEMM_BF16X3, COFI_GEMM_BF16X3 | COFI_GEMM_W_SPLIT | COFI_GEMM_A_SPLIT, COFI_GEMM_BF16X6 | COFI_GEMM_W_SPLIT,
                           COFI_GEMM_BF16X6, COFI_GEMM_BF16X6 | COFI_GEMM_F16X3}) {
        Plan p;
        if (plan_gemm(gemm_request(M, N, K, form, 0, 1, SIZE_MAX), p) == 0) need = std::max(need, p.ws_bytes);
    }
    return need;
}

extern "C" int cofi_gemm_f32_stat_slabs(int M, int N, int K) {
    if (M <= 0 || N <= 0 || K <= 0) return 0;
    return cofi_cdiv(M, 64);   // every path (64-row tiles, 128-row tiles in two halves, split-K reduction) emits 64-row slabs
}

extern "C" int cofi_gemm_f32(const float *A, int lda, const float *W, int ldw, float *C, int ldc, int M, int N, int K,
                             const float *bias, const float *rowdiv, int act, void *ws, size_t ws_bytes, cofi_stream_t stream) {
    return gemm_entry(A, lda, nullptr, W, ldw, C, ldc, M, N, K, bias, rowdiv, act, nullptr, 1, ws, ws_bytes, 1, stream);
}

extern "C" int cofi_gemm_f32_colstats(const float *A, int lda, const float *W, int ldw, float *C, int ldc, int M, int N, int K,
                                      const float *bias, const float *rowdiv, int act, float *colpart, void *ws, size_t ws_bytes,
                                      cofi_stream_t stream) {
    return gemm_entry(A, lda, nullptr, W, ldw, C, ldc, M, N, K, bias, rowdiv, act, colpart, 1, ws, ws_bytes, 1, stream);
}

extern "C" int cofi_gemm_f32_fused(const float *A, int lda, const cofi_norm_desc_t *a_norm, const float *W, int ldw, float *C, int ldc,
                                   int M, int N, int K, const float *bias, const float *rowdiv, int act, float *colpart, int stat_width,
                                   void *ws, size_t ws_bytes, int frames, cofi_stream_t stream) {
    return gemm_entry(A, lda, a_norm, W, ldw, C, ldc, M, N, K, bias, rowdiv, act, colpart, stat_width, ws, ws_bytes, frames, stream);
}

extern "C" int cofi_gemm_f32_fused_res(const float *A, int lda, const cofi_norm_desc_t *a_norm, const float *W, int ldw, float *C, int ldc,
                                       int M, int N, int K, const float *bias, const float *rowdiv, int act, float *colpart, int stat_width,
                                       void *ws, size_t ws_bytes, int frames, const float *res, int ldr, const int32_t *res_idx,
                                       int res_idx_stride, int res_rows, cofi_stream_t stream) {
    return gemm_entry(A, lda, a_norm, W, ldw, C, ldc, M, N, K, bias, rowdiv, act, colpart, stat_width, ws, ws_bytes, frames, stream, res, ldr,
                      res_idx, res_idx_stride, res_rows);
}

extern "C" int cofi_gemm_f32_layernorm(const float *A, int lda, const float *W, int ldw, float *C, int ldc, int M, int N, int K,
                                       const float *bias, const float *gamma, const float *beta, float eps, int relu, const float *res,
                                       int ldr, void *ws, size_t ws_bytes, cofi_stream_t stream) {
    if (int rc = check_common(A, lda, W, ldw, C, ldc, M, N, K)) return rc;
    if (!gamma || !beta || N > 128 || (res && ldr < N)) return COFI_EINVAL;   // (N: refused for an empty problem too, which is never planned)
    if (M == 0) return 0;
    PlanRequest rq = layernorm_request(M, N, K, relu, ws ? ws_bytes : 0);
    rq.operands_ok = !(rq.wsplit && (ldw & 7));
    Plan p;
    if (int rc = plan_gemm(rq, p)) return rc;
    GemmArgs g{};
    g.A = A; g.W = W; g.C = C; g.bias = bias; g.ws = (float *)ws; g.ln_gamma = gamma; g.ln_beta = beta; g.res = res;
    g.lda = lda; g.ldw = ldw; g.ldc = ldc; g.ldr = ldr; g.M = M; g.N = N; g.K = K; g.ksplit = 1; g.ln_relu = rq.act; g.ln_eps = eps;
    g.bf16x3 = rq.arith; g.wsplit = rq.wsplit; g.w_lo_off = (long)N * ldw; g.cv_Pout = 1;
    return launch(g, p, cofi_s(stream));
}

extern "C" int cofi_conv2d_nhwc(const float *x, int ldx, int H, int W, int Cin, const float *Wt, int Cout, int ks, int stride, int pad,
                                const float *bias, const float *res, int ldr, int act, float *y, int ldy, float *colpart, void *ws,
                                size_t ws_bytes, int frames, cofi_stream_t stream) {
    return conv_entry(x, ldx, nullptr, H, W, Cin, Wt, Cout, ks, stride, pad, bias, res, ldr, act, 0, y, ldy, colpart, 1, ws, ws_bytes, frames, stream);
}

extern "C" int cofi_conv2d_nhwc_fused(const float *x, int ldx, const cofi_norm_desc_t *x_norm, int H, int W, int Cin, const float *Wt, int Cout,
                                      int ks, int stride, int pad, const float *bias, const float *res, int ldr, int act, int act_col0, float *y,
                                      int ldy, float *colpart, int stat_width, void *ws, size_t ws_bytes, int frames, cofi_stream_t stream) {
    return conv_entry(x, ldx, x_norm, H, W, Cin, Wt, Cout, ks, stride, pad, bias, res, ldr, act, act_col0, y, ldy, colpart, stat_width, ws,
                      ws_bytes, frames, stream);
}

extern "C" int cofi_split_bf16_planes(const float *W, int ldw, int N, int K, void *planes, int ldp, int nplanes, cofi_stream_t stream) {
    if (!W || !planes || N <= 0 || K <= 0 || ldw < K || ldp < K || (ldp & 7) || ((uintptr_t)planes & 15) || (nplanes != 2 && nplanes != 3)) return COFI_EINVAL;
    const size_t total = (size_t)N * (ldp >> 1);
    hipLaunchKernelGGL(split_planes_kernel, dim3((unsigned)((total + 255) / 256 > 4096 ? 4096 : (total + 255) / 256)), dim3(256), 0, cofi_s(stream),
                       W, ldw, N, K, (unsigned *)planes, ldp, nplanes);
    return cofi_launch_status();
}

// ---- tuning / test hooks, declared in include/cofi_hip_tune.h (not part of the drop-in ABI of include/cofi_hip.h).  Every override is
// state of the calling thread.
extern "C" int cofi_tune_force_planes(int cfg, int ksplit) {
    if (cfg < -2 || cfg >= kNumPlanesCfg || ksplit < 0) return COFI_EINVAL;
    g_force_pcfg = cfg; g_force_pks = ksplit;
    return 0;
}

// 256 x 128 bf16x6 kernel: mode 1 = on every eligible launch (ksplit 0 = chosen by big_plan), -1 = never, 0 = table + heuristic
extern "C" int cofi_tune_force_big(int mode, int ksplit) {
    if (mode < -1 || mode > 1 || ksplit < 0 || ksplit > 64) return COFI_EINVAL;
    g_force_big = mode; g_force_big_ks = ksplit;
    return 0;
}

extern "C" int cofi_tune_force_conv_direct(int mode) {
    if (mode < -1 || mode > 2) return COFI_EINVAL;
    g_force_direct = mode;
    return 0;
}

extern "C" int cofi_tune_big_debug(int flags) {   // 64: the generic row-wise epilogue (identical bits); 256: the four-wave f16x3 geometry (identical bits); other bits: unused
    g_big_dbg = flags;
    return 0;
}

// Diagnostic counter of gemm_f16_big_kernel: tiles re-split because they left the fp16 window of their panel's scale (all launches since the
// last reset).  reset != 0 zeroes it after reading.  Synchronises the device.
extern "C" long cofi_tune_f16x3_resplit_events(int reset) {
    unsigned long long v = 0;
    if (hipMemcpyFromSymbol(&v, HIP_SYMBOL(g_f16_resplit_events), sizeof(v), 0, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    if (reset) {
        const unsigned long long z = 0;
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_f16_resplit_events), &z, sizeof(z), 0, hipMemcpyHostToDevice) != hipSuccess) return -1;
    }
    return (long)v;
}

// Host-side census (bench.py's roofline of a launch list that mixes the two arithmetics): contractions the CALLING THREAD enqueued on
// gemm_f16_big_kernel since the last reset -> their count, *flops = the sum of their 2 M N K.
extern "C" long cofi_tune_f16x3_launch_flops(int reset, double *flops) {
    const long n = g_f16_launches;
    if (flops) *flops = g_f16_flops;
    if (reset) { g_f16_launches = 0; g_f16_flops = 0.0; }
    return n;
}

extern "C" int cofi_tune_force_plan(int bm, int bn, int ksplit) {
    const bool ok = (bm == 0 && bn == 0) || ((bm == 64 || bm == 128) && (bn == 64 || bn == 128));   // 128 x 64: bf16x6 only (make_plan widens it otherwise)
    if (!ok || ksplit < 0) return COFI_EINVAL;
    g_force_bm = bm; g_force_bn = bn; g_force_ks = ksplit;
    return 0;
}

// The planner's answer for a request, under the calling thread's overrides; nothing is launched (no GPU needed).
extern "C" int cofi_tune_describe_gemm(int M, int N, int K, int act, int fused_ln, int pending_norm, int frames, size_t ws_bytes, cofi_plan_desc_t *out) {
    if (!out) return COFI_EINVAL;
    Plan p{};
    return describe(plan_gemm(fused_ln ? layernorm_request(M, N, K, act, ws_bytes) : gemm_request(M, N, K, act, pending_norm, frames, ws_bytes), p), p, out);
}

extern "C" int cofi_tune_describe_conv(int H, int W, int Cin, int Cout, int ks, int stride, int pad, int ldx, int act, int pending_norm, int frames,
                                       size_t ws_bytes, cofi_plan_desc_t *out) {
    if (!out) return COFI_EINVAL;
    PlanRequest r = conv_request(H, W, Cin, Cout, ks, stride, pad, ldx, act, pending_norm, frames, ws_bytes);
    Plan p{};
    return describe(plan_conv(r, p), p, out);
}
