// The validation pass of train.py on the device: the label gathers of a stack-mode mode='val' forward (network.py:137-141 for B
// frames in one launch) and the monitors train.py computes from a forward's outputs - test_acc's top-k coarse-descriptor recall
// (train.py:72-101), the fine-match recall (train.py:268-280) and the pc_score statistics (train.py:256-259) - for every frame of a
// submission in one launch, with no host read: capturable in a hipGraph.
// Integer results (counts, n_true, fine_hits) do not depend on any summation order; the floating-point ones (dist, score statistics)
// are computed by fixed-order loops and shuffles, so a replay is bit-equal to the eager call.
#include "match_parts.h"

namespace {

constexpr int VAL_NT = 256, VAL_NW = VAL_NT / 64;
constexpr int VAL_MAXK = 128, VAL_MAXC = 128, VAL_MAXTOP = 8, VAL_CH = 16;   // key points, coarse channels, top-k range, channels staged per step

__device__ __forceinline__ long long val_label(const void *p, int is64, size_t i) {
    return is64 ? ((const long long *)p)[i] : (long long)((const int32_t *)p)[i];
}
__device__ __forceinline__ int val_index(const void *p, int is64, size_t i, int n) {   // a label index, kept inside [0, n)
    const long long v = val_label(p, is64, i);
    return (int)(v < 0 ? 0 : (v >= n ? n - 1 : v));
}

// ---------------------------------------------------------------------------------------------- label gathers of a val-mode forward
// block (k, f): patches[f, k] (C, 16) = the 4 x 4 window of frame f's pixel-major fine map whose left top is centre - 2 (network.py:213,
// size / 2 = 2; patch_window, the gather of cofi_extract_patches_nhwc, with a 64-bit origin: a label anywhere in int64 gives zeros),
// fine_pc[f, k] = row inline_idx[f, k] of frame f's fine point descriptors (zero row for an index outside [0, N1))
__global__ __launch_bounds__(VAL_NT) void val_gather_kernel(const float *fmap, int ldf, int C, int H2, int W2, const float *fpc, int ldfpc,
                                                            int N1, const void *centers, const void *inline_idx, int is64, int K,
                                                            float *patches, float *fine_pc) {
    const int k = blockIdx.x, f = blockIdx.y;
    const long long cx = val_label(centers, is64, ((size_t)f * 2) * K + k), cy = val_label(centers, is64, ((size_t)f * 2 + 1) * K + k);
    float *po = patches + ((size_t)f * K + k) * C * 16;
    patch_window(fmap + (size_t)f * H2 * W2 * ldf, ldf, C, H2, W2, cx - 2, cy - 2, (int)threadIdx.x, VAL_NT,
                 [&](int c, int t, float v) { po[(size_t)c * 16 + t] = v; });
    const long long row = val_label(inline_idx, is64, (size_t)f * K + k);
    const bool ok = row >= 0 && row < N1;
    for (int c = threadIdx.x; c < C; c += VAL_NT)
        fine_pc[((size_t)f * K + k) * C + c] = ok ? fpc[((size_t)f * N1 + (size_t)row) * ldfpc + c] : 0.f;
}

// ---------------------------------------------------------------------------------------------- monitors
struct ValArgs {
    const float *img_desc, *pc_desc;   // (B, C, T) / (B, C, N4) channel-major
    const float *points4, *pc_score;   // (B N4, 3) / (B N4)
    const float *patches, *fine_pc;    // (B, K, C2, 16) / (B, K, C2)
    const void *pc_kpt_idx, *pc_outline_idx, *img_kpt_idx, *fine_xy, *fine_center;   // (B, K) x 3, (B, 2, K) x 2
    const float *K4, *P;               // (B, 3, 3) / (B, 4, 4)
    int32_t *counts, *n_true, *fine_hits;
    float *score_stats, *dist_out, *mask_out;
    int is64, K, C, T, W8, N4, C2, topk;
    float dist_thres;
};

// float bits -> unsigned whose order is the floats' order
__device__ __forceinline__ unsigned val_ordered(float v) {
    const unsigned b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float val_unordered(unsigned o) { return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o); }

// train.py:84: sqrt(dx^2 + dy^2) <= dist_thres.  The ONE place the mask is evaluated (the debug output and the true set both call it),
// every operation a separately rounded one whatever the compiler's contraction setting
__device__ __forceinline__ bool val_mask(float ix, float iy, float px, float py, float thres) {
    const float dx = __fsub_rn(ix, px), dy = __fsub_rn(iy, py);
    return __fsqrt_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy))) <= thres;
}

// LDS of the coarse workgroup, in floats: dist tile, true-value list, the staged descriptor chunk, per-key-point tables
__host__ __device__ constexpr size_t val_lds_floats(int K, int KP) {
    return (size_t)2 * K * K + (size_t)2 * VAL_CH * KP + (size_t)K * VAL_MAXTOP + 6 * (size_t)K;
}

// Frame f = blockIdx.x.  blockIdx.y == 0: the coarse part (train.py:72-101); blockIdx.y == 1: fine recall and score statistics.
// R = register tile edge: thread (ty, tx) of the 16 x 16 layout owns dist[ty + 16 r][tx + 16 q], r, q < R; KP = 16 R >= K.
template <int R>
__global__ __launch_bounds__(VAL_NT) void val_monitors_kernel(ValArgs a) {
    extern __shared__ float s_mem[];
    __shared__ int s_cnt[VAL_NW];
    __shared__ int s_hits[VAL_NW][VAL_MAXTOP];
    constexpr int KP = 16 * R;
    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int K = a.K;
    if (blockIdx.y == 1) {
        // ---- fine recall (train.py:268-280): per key point the pick of cofi_fine_match (its fine_cosine16 + argmax16) against
        // relative_index = (fine_xy - centre + 2) folded as y * 4 + x
        int hits = 0;
        for (int k = wave; k < K; k += VAL_NW) {
            const float *pt = a.patches + ((size_t)f * K + k) * a.C2 * 16, *pf = a.fine_pc + ((size_t)f * K + k) * a.C2;
            const int bi = argmax16(fine_cosine16([&](int c, int pxl) { return pt[(size_t)c * 16 + pxl]; }, [&](int c) { return pf[c]; }, a.C2, lane).sim(), lane);
            const size_t ix = ((size_t)f * 2) * K + k, iy = ((size_t)f * 2 + 1) * K + k;
            const long long rx = val_label(a.fine_xy, a.is64, ix) - val_label(a.fine_center, a.is64, ix) + 2;
            const long long ry = val_label(a.fine_xy, a.is64, iy) - val_label(a.fine_center, a.is64, iy) + 2;
            hits += ((long long)bi == ry * 4 + rx) ? 1 : 0;   // wave-uniform after the arg-max
        }
        if (lane == 0) s_cnt[wave] = hits;
        __syncthreads();
        if (tid == 0) {
            int tot = 0;
            for (int w = 0; w < VAL_NW; ++w) tot += s_cnt[w];
            a.fine_hits[f] = tot;
        }
        // ---- pc_score statistics (train.py:256-259): wave 0 the in-line key points, wave 1 the out-line ones
        if (wave < 2) {
            const void *idx = wave == 0 ? a.pc_kpt_idx : a.pc_outline_idx;
            float mx = -INFINITY, mn = INFINITY;
            double sum = 0.0;
            for (int k = lane; k < K; k += 64) {
                const float s = a.pc_score[(size_t)f * a.N4 + val_index(idx, a.is64, (size_t)f * K + k, a.N4)];
                mx = fmaxf(mx, s);
                mn = fminf(mn, s);
                sum += (double)s;
            }
            mx = wave_max(mx);
            mn = -wave_max(-mn);
            sum = wave_sum_d(sum);
            if (lane == 0) {
                float *o = a.score_stats + (size_t)f * 6 + 3 * wave;
                o[0] = mx; o[1] = mn; o[2] = (float)(sum / (double)K);
            }
        }
        return;
    }
    // ---------------------------------------------------------------- coarse part
    float *s_dist = s_mem;                          // (K, K)
    float *s_true = s_dist + (size_t)K * K;         // up to K * K values
    float *s_a = s_true + (size_t)K * K;            // (VAL_CH, KP) image descriptors of the chunk, key point minor
    float *s_b = s_a + VAL_CH * KP;                 // (VAL_CH, KP) point descriptors
    float *s_cand = s_b + VAL_CH * KP;              // (K, VAL_MAXTOP) the smallest values of every row, ascending
    float *s_ix = s_cand + (size_t)K * VAL_MAXTOP, *s_iy = s_ix + K, *s_px = s_iy + K, *s_py = s_px + K;
    int *s_ii = (int *)(s_py + K), *s_pi = s_ii + K;
    const float *img = a.img_desc + (size_t)f * a.C * a.T, *pc = a.pc_desc + (size_t)f * a.C * a.N4;
    // ---- labels, pixel coordinates, projection (train.py:73,78,80-82): proj = K_4 (R x + t), pc_xy = proj[:2] / proj[2]
    for (int k = tid; k < K; k += VAL_NT) {
        const int ii = val_index(a.img_kpt_idx, a.is64, (size_t)f * K + k, a.T);
        const int pi = val_index(a.pc_kpt_idx, a.is64, (size_t)f * K + k, a.N4);
        s_ii[k] = ii;
        s_pi[k] = pi;
        s_ix[k] = (float)(ii % a.W8);
        s_iy[k] = (float)(ii / a.W8);
        const float *x = a.points4 + ((size_t)f * a.N4 + pi) * 3, *P = a.P + (size_t)f * 16, *Km = a.K4 + (size_t)f * 9;
        float cam[3], pr[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) cam[r] = fmaf(P[4 * r + 2], x[2], fmaf(P[4 * r + 1], x[1], P[4 * r] * x[0])) + P[4 * r + 3];
#pragma unroll
        for (int r = 0; r < 3; ++r) pr[r] = fmaf(Km[3 * r + 2], cam[2], fmaf(Km[3 * r + 1], cam[1], Km[3 * r] * cam[0]));
        s_px[k] = pr[0] / pr[2];
        s_py[k] = pr[1] / pr[2];
    }
    __syncthreads();
    // ---- <img_i, pc_j> over the channels in ascending order: one fmaf chain per entry
    const int ty = tid >> 4, tx = tid & 15;
    float acc[R][R];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int q = 0; q < R; ++q) acc[r][q] = 0.f;
    for (int c0 = 0; c0 < a.C; c0 += VAL_CH) {
        for (int e = tid; e < VAL_CH * KP; e += VAL_NT) {
            const int c = e / KP, k = e - c * KP;
            const bool ok = k < K && c0 + c < a.C;
            s_a[e] = ok ? img[(size_t)(c0 + c) * a.T + s_ii[k]] : 0.f;
            s_b[e] = ok ? pc[(size_t)(c0 + c) * a.N4 + s_pi[k]] : 0.f;
        }
        __syncthreads();
#pragma unroll 4
        for (int c = 0; c < VAL_CH; ++c) {
            float av[R], bv[R];
#pragma unroll
            for (int r = 0; r < R; ++r) { av[r] = s_a[c * KP + ty + 16 * r]; bv[r] = s_b[c * KP + tx + 16 * r]; }
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
                for (int q = 0; q < R; ++q) acc[r][q] = fmaf(av[r], bv[q], acc[r][q]);
        }
        __syncthreads();
    }
    // ---- dist = 1 - <.,.> into the tile (train.py:86); the optional debug copies of dist and of the mask (train.py:84)
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int q = 0; q < R; ++q) {
            const int i = ty + 16 * r, j = tx + 16 * q;
            if (i < K && j < K) {
                const float d = 1.0f - acc[r][q];
                s_dist[(size_t)i * K + j] = d;
                if (a.dist_out) a.dist_out[((size_t)f * K + i) * K + j] = d;
                if (a.mask_out) a.mask_out[((size_t)f * K + i) * K + j] = val_mask(s_ix[i], s_iy[i], s_px[j], s_py[j], a.dist_thres) ? 1.f : 0.f;
            }
        }
    __syncthreads();
    // ---- the topk smallest values of every row in ascending order (torch.sort, train.py:92): one wave per row, (value, column) keys
    for (int i = wave; i < K; i += VAL_NW) {
        unsigned long long k0 = ~0ull, k1 = ~0ull;
        if (lane < K) k0 = ((unsigned long long)val_ordered(s_dist[(size_t)i * K + lane]) << 32) | (unsigned)lane;
        if (lane + 64 < K) k1 = ((unsigned long long)val_ordered(s_dist[(size_t)i * K + lane + 64]) << 32) | (unsigned)(lane + 64);
        for (int p = 0; p < a.topk; ++p) {
            const unsigned long long m = wave_min_key(k0 < k1 ? k0 : k1);
            if (lane == 0) s_cand[i * VAL_MAXTOP + p] = val_unordered((unsigned)(m >> 32));
            if (k0 == m) k0 = ~0ull;   // keys are unique (the column is part of them): exactly one entry leaves
            if (k1 == m) k1 = ~0ull;
        }
    }
    // ---- the true set (train.py:89-91): values dist[i, j] with mask[i, j] set and dist[i, j] != 0, compacted in row-major order
    int base = 0;
    for (int e0 = 0; e0 < K * K; e0 += VAL_NT) {
        const int e = e0 + tid;
        bool ok = false;
        float d = 0.f;
        if (e < K * K) {
            const int i = e / K, j = e - i * K;
            d = s_dist[e];
            ok = val_mask(s_ix[i], s_iy[i], s_px[j], s_py[j], a.dist_thres) && d != 0.f;
        }
        compact_chunk<VAL_NW>(ok, lane, wave, s_cnt, base, [&](int pos) { s_true[pos] = d; });
    }
    const int n_true = base;
    // ---- membership BY VALUE (train.py:95-101: `candidate in true_value_list`): one wave per candidate scans the list
    int hit[VAL_MAXTOP];
#pragma unroll
    for (int p = 0; p < VAL_MAXTOP; ++p) hit[p] = 0;
    for (int i = wave; i < K; i += VAL_NW) {
#pragma unroll
        for (int p = 0; p < VAL_MAXTOP; ++p) {
            if (p < a.topk) {
                const float v = s_cand[i * VAL_MAXTOP + p];
                bool found = false;
                for (int t = lane; t < n_true; t += 64) found = found || (s_true[t] == v);
                hit[p] += __ballot(found) != 0ull ? 1 : 0;
            }
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int p = 0; p < VAL_MAXTOP; ++p) s_hits[wave][p] = hit[p];
    }
    __syncthreads();
    if (tid < a.topk) {   // counts[k - 1]: the candidates among the first k of every row
        int tot = 0;
        for (int p = 0; p <= tid; ++p)
            for (int w = 0; w < VAL_NW; ++w) tot += s_hits[w][p];
        a.counts[(size_t)f * a.topk + tid] = tot;
    }
    if (tid == 0) a.n_true[f] = n_true;
}

template <int R>
int val_launch(const ValArgs &a, int frames, hipStream_t stream) {
    const size_t bytes = val_lds_floats(a.K, 16 * R) * sizeof(float);
    if (bytes > 48 * 1024) {   // beyond the default dynamic LDS limit of a launch: raised once per device (the limit only grows, so
        static int raised[64];   // concurrent first calls at worst both set it), not again inside a stream capture
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return COFI_EINVAL;
        if (raised[dev] < (int)bytes) {
            const hipError_t e = hipFuncSetAttribute((const void *)val_monitors_kernel<R>, hipFuncAttributeMaxDynamicSharedMemorySize, 159 * 1024);
            if (e != hipSuccess) return (int)e;
            raised[dev] = 159 * 1024;
        }
    }
    hipLaunchKernelGGL(val_monitors_kernel<R>, dim3(frames, 2), dim3(VAL_NT), bytes, stream, a);
    return cofi_launch_status();
}

}  // namespace

extern "C" size_t cofi_val_monitors_workspace(int K, int frames) {
    (void)K; (void)frames;
    return 0;   // the distance tile, the true-value list and the candidates live in LDS
}

extern "C" int cofi_val_gather(const float *fmap, int ldf, int C, int H2, int W2, const float *fine_pc_map, int ldfpc, int N1,
                               const void *centers, const void *inline_idx, int idx_is_i64, int K, int frames, float *patches,
                               float *fine_pc, cofi_stream_t stream) {
    if (!fmap || !fine_pc_map || !centers || !inline_idx || !patches || !fine_pc) return COFI_EINVAL;
    if (C <= 0 || H2 <= 0 || W2 <= 0 || N1 <= 0 || K <= 0 || frames <= 0 || frames > 65535 || ldf < C || ldfpc < C) return COFI_EINVAL;
    hipLaunchKernelGGL(val_gather_kernel, dim3(K, frames), dim3(VAL_NT), 0, cofi_s(stream), fmap, ldf, C, H2, W2, fine_pc_map, ldfpc, N1,
                       centers, inline_idx, idx_is_i64, K, patches, fine_pc);
    return cofi_launch_status();
}

extern "C" int cofi_val_monitors(const float *img_desc, const float *pc_desc, int C, int T, int W8, int N4, const float *points4,
                                 const float *pc_score, const float *patches, const float *fine_pc, int C2, const void *pc_kpt_idx,
                                 const void *pc_outline_idx, const void *coarse_img_kpt_idx, const void *fine_xy,
                                 const void *fine_center_kpt_coors, int idx_is_i64, const float *K_4, const float *P, float dist_thres,
                                 int K, int frames, int topk, int32_t *counts, int32_t *n_true, int32_t *fine_hits, float *score_stats,
                                 float *dist_out, float *mask_out, void *ws, size_t ws_bytes, cofi_stream_t stream) {
    (void)ws; (void)ws_bytes;
    if (!img_desc || !pc_desc || !points4 || !pc_score || !patches || !fine_pc || !pc_kpt_idx || !pc_outline_idx || !coarse_img_kpt_idx ||
        !fine_xy || !fine_center_kpt_coors || !K_4 || !P || !counts || !n_true || !fine_hits || !score_stats)
        return COFI_EINVAL;
    if (C <= 0 || T <= 0 || W8 <= 0 || N4 <= 0 || C2 <= 0 || K <= 0 || frames <= 0 || topk <= 0 || topk > VAL_MAXTOP || topk > K) return COFI_EINVAL;
    if (K > VAL_MAXK || C > VAL_MAXC) return COFI_EUNSUPPORTED;
    ValArgs a{img_desc, pc_desc, points4, pc_score, patches, fine_pc, pc_kpt_idx, pc_outline_idx, coarse_img_kpt_idx, fine_xy,
              fine_center_kpt_coors, K_4, P, counts, n_true, fine_hits, score_stats, dist_out, mask_out,
              idx_is_i64, K, C, T, W8, N4, C2, topk, dist_thres};
    const int r = cofi_cdiv(K, 16);
    if (r <= 2) return val_launch<2>(a, frames, cofi_s(stream));
    if (r <= 4) return val_launch<4>(a, frames, cofi_s(stream));
    if (r <= 6) return val_launch<6>(a, frames, cofi_s(stream));
    return val_launch<8>(a, frames, cofi_s(stream));
}
