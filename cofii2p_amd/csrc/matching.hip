// Coarse super-point -> super-pixel matching and 4x4 patch fine matching with no host round trip.
// Reference: model/network.py:145-161 (threshold loop), :167-187 (`fine_process`), :206-226
// (`extract_patch`), evaluation/eval_all.py:99-105 (fine matching in the caller).
// The match count stays on the device (count_dev); downstream kernels are launched at capacity and
// read it, so the only host synchronisation of a test-mode forward is the final read of the count.
#include "match_parts.h"

namespace {

// pix[n] = argmin_p (1 - sim[n,p]), first index on ties (torch.argmin).  One wave per row.
__global__ __launch_bounds__(256) void row_argmin_1m_kernel(const float *sim, int lds, int N, int P, int32_t *pix) {
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;
    const int lane = threadIdx.x & 63;
    float best = INFINITY;
    int bi = 0x7fffffff;
    for (int p = lane; p < P; p += 64) {
        const float d = 1.0f - sim[(size_t)n * lds + p];
        if (d < best) { best = d; bi = p; }  // strict: keeps the lowest p of this lane
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (ob < best || (ob == best && oi < bi)) { best = ob; bi = oi; }
    }
    if (lane == 0) pix[n] = bi;
}

struct SelArgs {
    const float *score;
    const int32_t *pix;
    int32_t *sel, *count;
    float *xy;
    int N, W8, H8, n_thr, min_matches, xmax, ymax;
    float thr[64];
};

// one workgroup per frame (stack mode: frame f reads score / pix rows [f N, (f + 1) N) and owns sel[f], xy[f] (2, N), count[f]):
// threshold search + ordered compaction (ascending point index).  256 threads: a 1024-thread workgroup needs a whole CU's wave slots
// and waits for one to drain while other submissions' kernels fill the chip (86 us on average at batch 16, round 4 - for 5 us of work)
constexpr int SEL_NT = 256, SEL_NW = SEL_NT / 64;
__global__ __launch_bounds__(SEL_NT) void select_matches_kernel(SelArgs a) {
    __shared__ int s_cnt[SEL_NW];
    __shared__ int s_thr;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int f = blockIdx.x;
    a.score += (size_t)f * a.N; a.pix += (size_t)f * a.N; a.sel += (size_t)f * a.N; a.xy += (size_t)f * 2 * a.N; a.count += 2 * f;
    // pass 1: find the first threshold with enough survivors
    if (tid == 0) s_thr = -1;
    __syncthreads();
    for (int t = 0; t < a.n_thr; ++t) {
        int c = 0;
        for (int n = tid; n < a.N; n += SEL_NT) {
            const int p = a.pix[n];
            const int x = p % a.W8, y = p / a.W8;
            const bool ok = a.score[n] >= a.thr[t] && x >= 2 && x <= a.xmax && y >= 2 && y <= a.ymax;
            c += ok ? 1 : 0;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
        if (lane == 0) s_cnt[wave] = c;
        __syncthreads();
        int tot = 0;
        for (int w = 0; w < SEL_NW; ++w) tot += s_cnt[w];
        __syncthreads();
        if (tot >= a.min_matches) {
            if (tid == 0) s_thr = t;
            break;  // uniform: every thread computed the same tot
        }
    }
    __syncthreads();
    const int tsel = s_thr;
    if (tsel < 0) {
        if (tid == 0) { a.count[0] = 0; a.count[1] = -1; }
        return;
    }
    const float thr = a.thr[tsel];
    // pass 2: ordered compaction in chunks of SEL_NT points
    int base = 0;
    for (int n0 = 0; n0 < a.N; n0 += SEL_NT) {
        const int n = n0 + tid;
        bool ok = false;
        int x = 0, y = 0;
        if (n < a.N) {
            const int p = a.pix[n];
            x = p % a.W8; y = p / a.W8;
            ok = a.score[n] >= thr && x >= 2 && x <= a.xmax && y >= 2 && y <= a.ymax;
        }
        compact_chunk<SEL_NW>(ok, lane, wave, s_cnt, base, [&](int pos) {
            a.sel[pos] = n;
            a.xy[pos] = (float)x;
            a.xy[a.N + pos] = (float)y;
        });
    }
    if (tid == 0) { a.count[0] = base; a.count[1] = tsel; }
}

__global__ void gather_points_sel_kernel(const float *pts, const int32_t *sel, const int32_t *count_dev, int cap, float *out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int n = min(*count_dev, cap);
    if (i >= n * 3) return;
    out[i] = pts[3 * (size_t)sel[i / 3] + (i % 3)];
}

// patches[i, c, r*4 + w] = fmap[(4*y - 2 + r) * W2 + 4*x - 2 + w, c]: fmap row (y*W2 + x) holds the C channels of a pixel
__global__ void extract_patches_nhwc_kernel(const float *fmap, int ldf, int C, int H2, int W2, const float *xy, int ldxy, float cscale,
                                            const int32_t *count_dev, int cap, float *patches) {
    const int i = blockIdx.x;
    if (i >= min(*count_dev, cap)) return;
    patch_window(fmap, ldf, C, H2, W2, patch_origin(xy[i], cscale), patch_origin(xy[ldxy + i], cscale), (int)threadIdx.x, (int)blockDim.x,
                 [&](int c, int t, float v) { patches[((size_t)i * C + c) * 16 + t] = v; });
}

__global__ void gather_rows_sel_kernel(const float *x, int ldx, int C, const int32_t *row_idx, const int32_t *count_dev, int cap,
                                       float *out, int ldo) {
    const int i = blockIdx.x;
    if (i >= min(*count_dev, cap)) return;
    const size_t r = (size_t)row_idx[i];
    for (int c = threadIdx.x; c < C; c += blockDim.x) out[(size_t)i * ldo + c] = x[r * ldx + c];
}

// one wave per match: 16 cosine similarities, argmax, fine_xy
__global__ __launch_bounds__(64) void fine_match_kernel(const float *patches, const float *pcf, int ldp, int C, const float *xy,
                                                        int ldxy, float cscale, const int32_t *count_dev, int cap, float *fine_xy,
                                                        int32_t *best) {
    const int i = blockIdx.x;
    if (i >= min(*count_dev, cap)) return;
    const int lane = threadIdx.x;
    const int bi = argmax16(fine_cosine16([&](int c, int pxl) { return patches[((size_t)i * C + c) * 16 + pxl]; },
                                          [&](int c) { return pcf[(size_t)i * ldp + c]; }, C, lane).sim(), lane);
    if (lane == 0) {
        best[i] = bi;
        const float2 f = fine_xy_pair(xy[i], xy[ldxy + i], cscale, bi);
        fine_xy[i] = f.x;
        fine_xy[cap + i] = f.y;
    }
}

// Everything of a test-mode forward that follows the match selection (network.py:153-161 + eval_all.py:99-105), one workgroup per
// accepted match i (count read on the device): the coarse point, its nearest stage-1 node (point2node, network.py:250-264: canonical
// distance, lowest index on ties - the (distance, index) key of nearest_kernel), that node's fine descriptor, the 4 x 4 patch of the
// fine image map under the coarse pixel and the fine matching of the two.  Every step is the body the five stand-alone kernels above /
// in knn.hip run (match_parts.h: nearest_scan, patch_window, fine_cosine16, argmax16, fine_xy_pair), fed from LDS where they read
// global memory: bit-identical outputs, four launches fewer on a frame's chain.
struct FinishArgs {
    const float *pts4, *pts1, *fmap, *xy, *fpc;
    const int32_t *sel, *count;
    float *coarse_pts, *patches, *fine_pc, *fine_xy;
    int32_t *best;
    int N1, cap, ldf, C, H2, W2, ldxy, ldfpc, ldo;
    float cscale;
    int N4;   // stage-4 points per frame (stack mode: frame f = blockIdx.x / cap; every per-frame array advances by its own frame size)
    int cameras;   // rig submissions (cofi_match_finish_rig): `cameras` consecutive frames share cloud f / cameras - pts4, pts1 and fpc hold frames / cameras blocks
};
constexpr int FIN_MAXC = 128;

__global__ __launch_bounds__(256) void match_finish_kernel(FinishArgs a) {
    __shared__ u64 s_key[4];
    __shared__ float s_f[FIN_MAXC], s_p[FIN_MAXC * 16];
    const int f = blockIdx.x / a.cap, i = blockIdx.x - f * a.cap;
    a.count += 2 * f;
    if (i >= min(*a.count, a.cap)) return;
    const int cl = f / a.cameras;   // the frame's cloud: the only per-cloud operands are pts4, pts1 and fpc
    a.pts4 += (size_t)cl * a.N4 * 3; a.pts1 += (size_t)cl * a.N1 * 3; a.sel += (size_t)f * a.cap; a.xy += (size_t)f * 2 * a.ldxy;
    a.fmap += (size_t)f * a.H2 * a.W2 * a.ldf; a.fpc += (size_t)cl * a.N1 * a.ldfpc;
    a.coarse_pts += (size_t)f * a.cap * 3; a.patches += (size_t)f * a.cap * a.C * 16; a.fine_pc += (size_t)f * a.cap * a.ldo;
    a.fine_xy += (size_t)f * 2 * a.cap; a.best += (size_t)f * a.cap;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t n = (size_t)a.sel[i];
    const float qx = a.pts4[3 * n], qy = a.pts4[3 * n + 1], qz = a.pts4[3 * n + 2];
    if (tid < 3) a.coarse_pts[3 * (size_t)i + tid] = a.pts4[3 * n + tid];
    // nearest stage-1 node
    const u64 bestk = wave_min_key(nearest_scan<256>(a.pts1, a.N1, qx, qy, qz, tid));
    if (lane == 0) s_key[wave] = bestk;
    // the patch does not depend on the node: gathered while the keys settle
    const float cx = a.xy[i], cy = a.xy[a.ldxy + i];
    patch_window(a.fmap, a.ldf, a.C, a.H2, a.W2, patch_origin(cx, a.cscale), patch_origin(cy, a.cscale), tid, 256, [&](int c, int t, float v) {
        a.patches[((size_t)i * a.C + c) * 16 + t] = v;
        s_p[c * 16 + t] = v;
    });
    __syncthreads();
    const size_t node = (size_t)(unsigned)(umin64(umin64(s_key[0], s_key[1]), umin64(s_key[2], s_key[3])) & 0xffffffffu);
    for (int c = tid; c < a.C; c += 256) {
        const float v = a.fpc[node * a.ldfpc + c];
        a.fine_pc[(size_t)i * a.ldo + c] = v;
        s_f[c] = v;
    }
    __syncthreads();
    if (wave != 0) return;
    const int bi = argmax16(fine_cosine16([&](int c, int pxl) { return s_p[c * 16 + pxl]; }, [&](int c) { return s_f[c]; }, a.C, lane).sim(), lane);
    if (lane == 0) {
        a.best[i] = bi;
        const float2 fx = fine_xy_pair(cx, cy, a.cscale, bi);
        a.fine_xy[i] = fx.x;
        a.fine_xy[a.cap + i] = fx.y;
    }
}

// Sub-pixel refinement of the fine matches match_finish left: one wave per match i of frame f, REF_NW matches per
// workgroup.  The matched cell is the GEOMETRIC decode of best - column left + best % 4, row top + best / 4 of the fine map (fine_xy
// keeps the reference caller's transposed one) - and each axis gets the peak of the parabola through the cosine similarities of the
// descriptor with the cell and its two neighbours ON THE MAP, not in the patch.  No LDS, no barrier: a wave at or beyond the count
// leaves at once.
struct RefineArgs {
    const float *fmap, *xy, *fpc;
    const int32_t *best, *count;
    float *sub_xy, *peak;
    int ldf, C, H2, W2, ldxy, ldp, cap, vec;
    float cscale;
    int nb;   // workgroups per frame
};
constexpr int REF_NW = 4;

__global__ __launch_bounds__(64 * REF_NW) void fine_refine_kernel(RefineArgs a) {
    const int f = blockIdx.x / a.nb, i = (blockIdx.x - f * a.nb) * REF_NW + (int)(threadIdx.x >> 6);
    if (i >= min(a.count[2 * f], a.cap)) return;   // wave-uniform
    const int lane = threadIdx.x & 63;
    a.fmap += (size_t)f * a.H2 * a.W2 * a.ldf; a.xy += (size_t)f * 2 * a.ldxy; a.fpc += (size_t)f * a.cap * a.ldp;
    a.best += (size_t)f * a.cap; a.sub_xy += (size_t)f * 2 * a.cap; a.peak += (size_t)f * a.cap;
    const int bi = a.best[i];
    const int px = patch_origin(a.xy[i], a.cscale) + bi % 4, py = patch_origin(a.xy[a.ldxy + i], a.cscale) + bi / 4;
    float dx = 0.f, dy = 0.f, pk = 0.f;
    if (px >= 0 && px < a.W2 && py >= 0 && py < a.H2) {   // else a zero-padded patch cell won: nothing to refine
        const bool ax = px >= 1 && px <= a.W2 - 2, ay = py >= 1 && py <= a.H2 - 2;
        const float *c = a.fmap + ((size_t)py * a.W2 + (size_t)px) * a.ldf;
        const size_t up = (size_t)a.W2 * a.ldf;
        const float *const rows[5] = {c, ax ? c - a.ldf : nullptr, ax ? c + a.ldf : nullptr, ay ? c - up : nullptr, ay ? c + up : nullptr};
        float s[5];
        cosine_rows<5>(rows, a.fpc + (size_t)i * a.ldp, a.C, a.vec != 0, lane, s);
        if (ax) dx = parabola_offset(s[1], s[0], s[2]);
        if (ay) dy = parabola_offset(s[3], s[0], s[4]);
        pk = fabsf(s[0]) < INFINITY ? s[0] : 0.f;   // a NaN or Inf on the map must not reach the pose tail
    }
    if (lane == 0) {
        a.sub_xy[i] = (float)px + dx;
        a.sub_xy[a.cap + i] = (float)py + dy;
        a.peak[i] = pk;
    }
}

}  // namespace

extern "C" int cofi_fine_refine(const float *fmap, int ldf, int C, int H2, int W2, const float *coarse_xy, int ldxy, float center_scale,
                                const float *fine_pc, int ldp, const int32_t *best, const int32_t *count_dev, int cap, float *sub_xy,
                                float *peak, int frames, cofi_stream_t stream) {
    if (!fmap || !coarse_xy || !fine_pc || !best || !count_dev || !sub_xy || !peak) return COFI_EINVAL;
    if (C <= 0 || H2 <= 0 || W2 <= 0 || cap <= 0 || frames <= 0 || ldf < C || ldp < C || ldxy < cap) return COFI_EINVAL;
    const int nb = cofi_cdiv(cap, REF_NW);
    if ((long long)nb * frames > 0x7fffffffLL) return COFI_EINVAL;
    // 16-byte loads: both operands aligned and every row of either a whole number of 16-byte words after the first
    const int vec = ((reinterpret_cast<uintptr_t>(fmap) | reinterpret_cast<uintptr_t>(fine_pc)) % 16 == 0 && ldf % 4 == 0 && ldp % 4 == 0) ? 1 : 0;
    RefineArgs a{fmap, coarse_xy, fine_pc, best, count_dev, sub_xy, peak, ldf, C, H2, W2, ldxy, ldp, cap, vec, center_scale, nb};
    hipLaunchKernelGGL(fine_refine_kernel, dim3(nb * frames), dim3(64 * REF_NW), 0, cofi_s(stream), a);
    return cofi_launch_status();
}

extern "C" int cofi_match_finish_rig(const float *pts4, const float *pts1, int N1, const int32_t *sel, const int32_t *count_dev, int cap,
                                     const float *fmap, int ldf, int C, int H2, int W2, const float *coarse_xy, int ldxy, float center_scale,
                                     const float *fine_pc_all, int ldfpc, float *coarse_pts, float *patches, float *fine_pc, int ldo,
                                     float *fine_xy, int32_t *best, int N4, int frames, int cameras, cofi_stream_t stream) {
    if (!pts4 || !pts1 || !sel || !count_dev || !fmap || !coarse_xy || !fine_pc_all || !coarse_pts || !patches || !fine_pc || !fine_xy || !best)
        return COFI_EINVAL;
    if (N1 <= 0 || cap <= 0 || C <= 0 || H2 <= 0 || W2 <= 0 || ldf < C || ldfpc < C || ldo < C || N4 <= 0 || frames <= 0) return COFI_EINVAL;
    if (cameras <= 0 || frames % cameras) return COFI_EINVAL;
    if (C > FIN_MAXC) return COFI_EUNSUPPORTED;
    FinishArgs a{pts4, pts1, fmap, coarse_xy, fine_pc_all, sel, count_dev, coarse_pts, patches, fine_pc, fine_xy, best,
                 N1, cap, ldf, C, H2, W2, ldxy, ldfpc, ldo, center_scale, N4, cameras};
    hipLaunchKernelGGL(match_finish_kernel, dim3(cap * frames), dim3(256), 0, cofi_s(stream), a);
    return cofi_launch_status();
}

extern "C" int cofi_match_finish(const float *pts4, const float *pts1, int N1, const int32_t *sel, const int32_t *count_dev, int cap,
                                 const float *fmap, int ldf, int C, int H2, int W2, const float *coarse_xy, int ldxy, float center_scale,
                                 const float *fine_pc_all, int ldfpc, float *coarse_pts, float *patches, float *fine_pc, int ldo,
                                 float *fine_xy, int32_t *best, int N4, int frames, cofi_stream_t stream) {
    return cofi_match_finish_rig(pts4, pts1, N1, sel, count_dev, cap, fmap, ldf, C, H2, W2, coarse_xy, ldxy, center_scale, fine_pc_all, ldfpc,
                                 coarse_pts, patches, fine_pc, ldo, fine_xy, best, N4, frames, 1, stream);
}

extern "C" int cofi_row_argmin_1m(const float *sim, int lds, int N, int P, int32_t *pix, cofi_stream_t stream) {
    if (!sim || !pix || N <= 0 || P <= 0 || lds < P) return COFI_EINVAL;
    hipLaunchKernelGGL(row_argmin_1m_kernel, dim3(cofi_cdiv(N, 4)), dim3(256), 0, cofi_s(stream), sim, lds, N, P, pix);
    return cofi_launch_status();
}

extern "C" int cofi_select_matches(const float *score, const int32_t *pix, int N, int W8, int H8, int x_max, int y_max, const float *thr_host,
                                   int n_thr, int min_matches, int32_t *sel, float *coarse_xy, int32_t *count_dev, int frames, cofi_stream_t stream) {
    if (!score || !pix || !thr_host || !sel || !coarse_xy || !count_dev || N <= 0 || W8 <= 0 || H8 <= 0 || n_thr <= 0 || n_thr > 64 || frames <= 0)
        return COFI_EINVAL;
    SelArgs a;
    a.score = score; a.pix = pix; a.sel = sel; a.count = count_dev; a.xy = coarse_xy;
    a.N = N; a.W8 = W8; a.H8 = H8; a.n_thr = n_thr; a.min_matches = min_matches; a.xmax = x_max; a.ymax = y_max;
    for (int i = 0; i < 64; ++i) a.thr[i] = i < n_thr ? thr_host[i] : 0.f;
    hipLaunchKernelGGL(select_matches_kernel, dim3(frames), dim3(SEL_NT), 0, cofi_s(stream), a);
    return cofi_launch_status();
}

extern "C" int cofi_gather_points_sel(const float *pts, const int32_t *sel, const int32_t *count_dev, int cap, float *out,
                                      cofi_stream_t stream) {
    if (!pts || !sel || !count_dev || !out || cap <= 0) return COFI_EINVAL;
    hipLaunchKernelGGL(gather_points_sel_kernel, dim3(cofi_cdiv(cap * 3, 256)), dim3(256), 0, cofi_s(stream), pts, sel, count_dev, cap,
                       out);
    return cofi_launch_status();
}

extern "C" int cofi_extract_patches_nhwc(const float *fmap, int ldf, int C, int H2, int W2, const float *coarse_xy, int ldxy,
                                         float center_scale, const int32_t *count_dev, int cap, float *patches, cofi_stream_t stream) {
    if (!fmap || !coarse_xy || !count_dev || !patches || C <= 0 || H2 <= 0 || W2 <= 0 || cap <= 0 || ldf < C) return COFI_EINVAL;
    hipLaunchKernelGGL(extract_patches_nhwc_kernel, dim3(cap), dim3(256), 0, cofi_s(stream), fmap, ldf, C, H2, W2, coarse_xy, ldxy,
                       center_scale, count_dev, cap, patches);
    return cofi_launch_status();
}

extern "C" int cofi_gather_rows_sel(const float *x, int ldx, int C, const int32_t *row_idx, const int32_t *count_dev, int cap,
                                    float *out, int ldo, cofi_stream_t stream) {
    if (!x || !row_idx || !count_dev || !out || C <= 0 || cap <= 0 || ldx < C || ldo < C) return COFI_EINVAL;
    hipLaunchKernelGGL(gather_rows_sel_kernel, dim3(cap), dim3(64), 0, cofi_s(stream), x, ldx, C, row_idx, count_dev, cap, out, ldo);
    return cofi_launch_status();
}

extern "C" int cofi_fine_match(const float *patches, const float *pc_feats, int ldp, int C, const float *coarse_xy, int ldxy,
                               float center_scale, const int32_t *count_dev, int cap, float *fine_xy, int32_t *best,
                               cofi_stream_t stream) {
    if (!patches || !pc_feats || !coarse_xy || !count_dev || !fine_xy || !best || C <= 0 || cap <= 0 || ldp < C) return COFI_EINVAL;
    hipLaunchKernelGGL(fine_match_kernel, dim3(cap), dim3(64), 0, cofi_s(stream), patches, pc_feats, ldp, C, coarse_xy, ldxy,
                       center_scale, count_dev, cap, fine_xy, best);
    return cofi_launch_status();
}
