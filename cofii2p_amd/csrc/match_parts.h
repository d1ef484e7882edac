// The steps of the matching tail (model/network.py:153-161, :206-226, :250-264; evaluation/eval_all.py:99-105), each written ONCE and
// shared by its stand-alone kernel, the fused cofi_match_finish and the validation / loss kernels (matching.hip, knn.hip,
// validation.hip, loss.hip).  Every body is fed values or small accessors and never asks which caller it serves, so two kernels that
// share one produce the same bits by construction.
#pragma once
#include "knn_common.h"

namespace {

// Nearest-node scan: the calling thread's smallest (canonical distance, index) key over rows t, t + NT, ... of nodes (S, 3).
// 4 candidates per thread and round, all 12 loads issued before the first distance (a row past the end re-reads row S - 1 and is not
// counted): the scan is bound by the L2 round trip per round, not by arithmetic.  The key makes the result independent of the visiting
// order, hence of NT.
template <int NT>
__device__ __forceinline__ u64 nearest_scan(const float *nodes, int S, float qx, float qy, float qz, int t) {
    const float qq = canon_sqnorm(qx, qy, qz);
    u64 best = KEY_INF;
    for (int c0 = t; c0 < S; c0 += 4 * NT) {
        float px[4], py[4], pz[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int c = min(c0 + NT * u, S - 1);
            px[u] = nodes[3 * (size_t)c];
            py[u] = nodes[3 * (size_t)c + 1];
            pz[u] = nodes[3 * (size_t)c + 2];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int c = c0 + NT * u;
            const float d = canon_dist(qx, qy, qz, qq, px[u], py[u], pz[u], canon_sqnorm(px[u], py[u], pz[u]));
            if (c < S) best = umin64(best, ((u64)__float_as_uint(d) << 32) | (unsigned)c);
        }
    }
    return best;
}

// 4 x 4 window of a pixel-major map (row y * W2 + x = the C channels of a pixel) with left top (left, top), zero outside the map:
// sink(c, t, v) receives channel c of window pixel t = r * 4 + w once per element, thread tid of nt taking elements tid, tid + nt, ...
// I = integer type of the origin: long long where it comes from labels that may lie anywhere in int64.
template <typename I, typename Sink>
__device__ __forceinline__ void patch_window(const float *fmap, int ldf, int C, int H2, int W2, I left, I top, int tid, int nt, Sink sink) {
    for (int e = tid; e < C * 16; e += nt) {
        const int c = e % C, t = e / C, r = t >> 2, w = t & 3;   // lanes sweep channels: contiguous reads
        const I yy = top + r, xx = left + w;
        float v = 0.f;
        if (yy >= 0 && yy < H2 && xx >= 0 && xx < W2) v = fmap[((size_t)yy * W2 + (size_t)xx) * ldf + c];
        sink(c, t, v);
    }
}
// window origin of a coarse pixel coordinate v (network.py:213: centre - size / 2) ...
__device__ __forceinline__ int patch_origin(float v, float cscale) { return (int)floorf(v * cscale - 2.0f); }
// ... and the fine match of the coarse pixel (cx, cy) whose best window pixel is bi.  eval_all.py:103-105: x receives idx // 4 and y
// receives idx % 4 (kept as in the reference)
__device__ __forceinline__ float2 fine_xy_pair(float cx, float cy, float cscale, int bi) {
    return make_float2((cx * cscale - 2.0f) + (float)(bi / 4), (cy * cscale - 2.0f) + (float)(bi % 4));
}

// Cosine similarity (torch.cosine_similarity, eps 1e-8) of the 16 pixels of a (C, 16) patch against one C-channel descriptor, by one
// wave: lane = (pixel lane & 15, channel quarter lane >> 4); patch(c, pixel) and feat(c) supply the values.  Every lane ends with
// the sums of its pixel: dot, nx and ny (the clamped norms).
struct Cosine16 {
    float dot, nx, ny;
    __device__ __forceinline__ float sim() const { return dot / (nx * ny); }
};
template <typename Patch, typename Feat>
__device__ __forceinline__ Cosine16 fine_cosine16(Patch patch, Feat feat, int C, int lane) {
    const int pxl = lane & 15, part = lane >> 4;
    float dot = 0.f, nn = 0.f, pp = 0.f;
    for (int c = part; c < C; c += 4) {
        const float pv = patch(c, pxl), fv = feat(c);
        dot += pv * fv;
        nn += pv * pv;
        pp += fv * fv;
    }
    dot += __shfl_xor(dot, 16, 64); dot += __shfl_xor(dot, 32, 64);
    nn += __shfl_xor(nn, 16, 64); nn += __shfl_xor(nn, 32, 64);
    pp += __shfl_xor(pp, 16, 64); pp += __shfl_xor(pp, 32, 64);
    return {dot, fmaxf(sqrtf(nn), 1e-8f), fmaxf(sqrtf(pp), 1e-8f)};
}
// pixel with the largest similarity, the first one on ties (torch.argmax), in every lane
__device__ __forceinline__ int argmax16(float sim, int lane) {
    int bi = lane & 15;
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) {
        const float os = __shfl_xor(sim, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (os > sim || (os == sim && oi < bi)) { sim = os; bi = oi; }
    }
    return bi;
}

// Cosine similarity (the rule of fine_cosine16: each norm clamped at 1e-8) of NR rows of C floats against one descriptor row, by one
// wave.  rows[p] == nullptr (the same in every lane) stands for a row that is not read; its similarity is 0.  Lane l owns channels
// 4 l .. 4 l + 3, then + 256, ...: one 16-byte load per row and round where vec allows it (every row pointer 16-byte aligned; a round
// that ends past C is read float by float), and the SAME channels in the same order where it does not, so a lane's sums - and with the
// fixed butterfly the similarity - do not depend on vec, and rows that hold equal values give bit-equal similarities.
template <int NR>
__device__ __forceinline__ void cosine_rows(const float *const (&rows)[NR], const float *feat, int C, bool vec, int lane, float (&sim)[NR]) {
    float dot[NR], nn[NR], pp = 0.f;
#pragma unroll
    for (int p = 0; p < NR; ++p) dot[p] = nn[p] = 0.f;
    for (int c0 = 4 * lane; c0 < C; c0 += 256) {
        float fv[4], pv[NR][4];
        if (vec && c0 + 4 <= C) {
            const float4 t = *reinterpret_cast<const float4 *>(feat + c0);
            fv[0] = t.x; fv[1] = t.y; fv[2] = t.z; fv[3] = t.w;
#pragma unroll
            for (int p = 0; p < NR; ++p) {
                const float4 v = rows[p] ? *reinterpret_cast<const float4 *>(rows[p] + c0) : make_float4(0.f, 0.f, 0.f, 0.f);
                pv[p][0] = v.x; pv[p][1] = v.y; pv[p][2] = v.z; pv[p][3] = v.w;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const bool in = c0 + k < C;
                fv[k] = in ? feat[c0 + k] : 0.f;
#pragma unroll
                for (int p = 0; p < NR; ++p) pv[p][k] = in && rows[p] ? rows[p][c0 + k] : 0.f;
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            pp += fv[k] * fv[k];
#pragma unroll
            for (int p = 0; p < NR; ++p) {
                dot[p] += pv[p][k] * fv[k];
                nn[p] += pv[p][k] * pv[p][k];
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        pp += __shfl_xor(pp, o, 64);
#pragma unroll
        for (int p = 0; p < NR; ++p) {
            dot[p] += __shfl_xor(dot[p], o, 64);
            nn[p] += __shfl_xor(nn[p], o, 64);
        }
    }
    const float ny = fmaxf(sqrtf(pp), 1e-8f);
#pragma unroll
    for (int p = 0; p < NR; ++p) sim[p] = dot[p] / (fmaxf(sqrtf(nn[p]), 1e-8f) * ny);
}
// Offset in [-0.5, 0.5] of the peak of the parabola through the similarities sm, s0, sp at -1, 0, +1.  Where the three are not
// strictly concave the offset is half a cell towards the larger neighbour, 0 between equal ones.  Every comparison is false for a NaN:
// one among the three yields 0, and the clamp returns its bound where the quotient is one (Inf / Inf) - the result is always finite.
__device__ __forceinline__ float parabola_offset(float sm, float s0, float sp) {
    const float den = (sm - 2.0f * s0) + sp;
    if (den < 0.f) return fminf(fmaxf(0.5f * (sm - sp) / den, -0.5f), 0.5f);
    if (!(den >= 0.f)) return 0.f;
    return sp > sm ? 0.5f : (sp < sm ? -0.5f : 0.f);
}

// One chunk of an ordered compaction by a workgroup of NW waves: thread (wave, lane) holds the chunk's element 64 wave + lane, kept
// where ok.  store(slot) runs for every kept element, slots ascending from base in element order; base advances by the chunk's count.
// s_cnt: NW ints of LDS.  All threads call; ends on a barrier (s_cnt reusable, the stores visible to the workgroup).
template <int NW, typename Store>
__device__ __forceinline__ void compact_chunk(bool ok, int lane, int wave, int *s_cnt, int &base, Store store) {
    const unsigned long long m = __ballot(ok);
    if (lane == 0) s_cnt[wave] = __popcll(m);
    __syncthreads();
    int off = base, tot = 0;
    for (int w = 0; w < NW; ++w) {
        if (w < wave) off += s_cnt[w];
        tot += s_cnt[w];
    }
    if (ok) store(off + __popcll(m & ((1ull << lane) - 1ull)));
    base += tot;
    __syncthreads();
}

}  // namespace
