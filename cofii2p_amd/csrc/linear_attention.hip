// K6b  LoFTR linear attention (model/transformer/linear_attention.py:14-47, `LinearAttention.forward`) together with the token-axis query
// scaling of model/transformer/transformer.py:53, per frame and head (D == 32):
//
//   phi(x)  = x + 1 (x > 0), exp(x) otherwise                      elu(x) + 1
//   KV[d,v] = sum_s phi(k)[s,d] * (v[s,v] / S)        Ksum[d] = sum_s phi(k)[s,d]
//   Z[l]    = 1 / (sum_d phi(q')[l,d] * Ksum[d] + eps)             q' = q * q_colscale
//   out[l,v] = (sum_d phi(q')[l,d] * KV[d,v]) * Z[l] * S
//
// Three launches, all fp32 FMA (the products are 32 x 32 x S and L x 32 x 32 per head: about 8 flop per byte of K / V read):
//   summary  grid (source chunk of CHUNK rows, head, frame): the chunk's partial KV / Ksum -> its own slot of the workspace
//   fold     the slots of a (frame, head) summed in a fixed order -> the final slot
//   apply    grid (64-query block, head, frame): phi(q') against the final slot
// No floating-point atomics anywhere: the chunking depends on S alone and every sum has a fixed order, so a stacked call gives frame f the
// bits of the single-frame call on its slice, and two runs agree bit for bit.
//
// phi flushes exp() results below the smallest normal number (x < -87.3) to zero: a source whose keys are all very negative has KV = Ksum = 0
// exactly and out = 0 * (1 / eps) * S = 0, whatever the denormal mode of the build.
#include "common.h"

namespace {

constexpr int D = 32;              // head dimension
constexpr int CHUNK = 128;         // source rows per summary workgroup (two tiles: both in flight before the first is accumulated)
constexpr int TILE = 64;           // source rows staged in LDS at a time; query rows per apply workgroup
constexpr int SLOT = D * D + D;    // floats per slot: KV (d-major) then Ksum

__device__ __forceinline__ float phi(float x) { return x > 0.f ? x + 1.f : (x < -87.3f ? 0.f : expf(x)); }

__device__ __forceinline__ float4 phi4(float4 a) { return make_float4(phi(a.x), phi(a.y), phi(a.z), phi(a.w)); }

// slot index of (frame f, head h, chunk c); c == nchunk is the folded result
__device__ __forceinline__ size_t slot_of(int f, int H, int h, int nchunk, int c) { return (((size_t)f * H + h) * (nchunk + 1) + c) * SLOT; }

// thread t: KV[d = t / 8][4 * (t % 8) .. + 3] (and Ksum[d], kept by the thread with t % 8 == 0)
__global__ __launch_bounds__(256) void linear_attention_summary_kernel(const float *K, int ldk, const float *V, int ldv, int S, int H, int nchunk,
                                                                        float *ws) {
    __shared__ __attribute__((aligned(16))) float ks[TILE][D];
    __shared__ __attribute__((aligned(16))) float vs[TILE][D];
    const int c = blockIdx.x, h = blockIdx.y, f = blockIdx.z, t = threadIdx.x;
    const int s_begin = c * CHUNK, s_end = min(S, s_begin + CHUNK);
    const float fS = (float)S;
    const int d = t >> 3, v0 = (t & 7) * 4;
    float acc0 = 0.f, acc1 = 0.f, acc2 = 0.f, acc3 = 0.f, ksum = 0.f;
    // a tile = 64 rows x 8 float4 per operand: two per thread, held in registers from one tile ahead (the loads of tile i + 1 are in
    // flight while tile i is accumulated: a workgroup is a short serial chain, its time is load latency unless they overlap)
    float4 kraw[2], vraw[2];
    auto fetch = [&](int s0) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int e = t + 256 * i, r = e >> 3, q = (e & 7) * 4;
            kraw[i] = vraw[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (s0 + r < s_end) {
                const size_t row = (size_t)f * S + s0 + r;
                kraw[i] = *reinterpret_cast<const float4 *>(K + row * ldk + h * D + q);
                vraw[i] = *reinterpret_cast<const float4 *>(V + row * ldv + h * D + q);
            }
        }
    };
    fetch(s_begin);
    for (int s0 = s_begin; s0 < s_end; s0 += TILE) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int e = t + 256 * i, r = e >> 3, q = (e & 7) * 4;
            float4 kk = make_float4(0.f, 0.f, 0.f, 0.f), vv = kk;
            if (s0 + r < s_end) {   // (phi(0) = 1: a row past the end must be zeroed after the feature map, not before)
                kk = phi4(kraw[i]);
                vv = make_float4(vraw[i].x / fS, vraw[i].y / fS, vraw[i].z / fS, vraw[i].w / fS);
            }
            *reinterpret_cast<float4 *>(&ks[r][q]) = kk;
            *reinterpret_cast<float4 *>(&vs[r][q]) = vv;
        }
        __syncthreads();
        if (s0 + TILE < s_end) fetch(s0 + TILE);
#pragma unroll 8
        for (int r = 0; r < TILE; ++r) {   // rows past s_end hold zeros
            const float kd = ks[r][d];
            const float4 vv = *reinterpret_cast<const float4 *>(&vs[r][v0]);
            acc0 = fmaf(kd, vv.x, acc0);
            acc1 = fmaf(kd, vv.y, acc1);
            acc2 = fmaf(kd, vv.z, acc2);
            acc3 = fmaf(kd, vv.w, acc3);
            ksum += kd;
        }
        __syncthreads();
    }
    float *slot = ws + slot_of(f, H, h, nchunk, c);
    *reinterpret_cast<float4 *>(slot + d * D + v0) = make_float4(acc0, acc1, acc2, acc3);
    if ((t & 7) == 0) slot[D * D + d] = ksum;
}

// final slot = the chunk slots of a (frame, head) summed in a fixed order: wave g of a workgroup sums the chunks c = g, g + 4, ... of 64
// elements in ascending order (four independent chains of loads instead of one), then (p0 + p1) + (p2 + p3).  grid (ceil(SLOT / 64), frames * H)
__global__ __launch_bounds__(256) void linear_attention_fold_kernel(float *ws, int nchunk) {
    __shared__ float part[4][64];
    const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int e = blockIdx.x * 64 + lane;
    float *base = ws + (size_t)blockIdx.y * (nchunk + 1) * SLOT;
    float s = 0.f;
    if (e < SLOT) {
#pragma unroll 4
        for (int c = g; c < nchunk; c += 4) s += base[(size_t)c * SLOT + e];
    }
    part[g][lane] = s;
    __syncthreads();
    if (g == 0 && e < SLOT) base[(size_t)nchunk * SLOT + e] = (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]);
}

// thread t: query row t / 4 of the block, out columns 8 * (t % 4) .. + 7 of head h
__global__ __launch_bounds__(256) void linear_attention_apply_kernel(const float *Q, int ldq, const float *q_colscale, int L, int S, int H, int nchunk,
                                                                      float eps, const float *ws, float *O, int ldo) {
    __shared__ __attribute__((aligned(16))) float kv[SLOT];
    __shared__ float qs[TILE][D + 1];
    const int h = blockIdx.y, f = blockIdx.z, t = threadIdx.x;
    const int l0 = blockIdx.x * TILE;
    const float *slot = ws + slot_of(f, H, h, nchunk, nchunk);
    for (int i = t; i < SLOT; i += 256) kv[i] = slot[i];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int e = t + 256 * i, r = e >> 3, q = (e & 7) * 4;
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
        if (l0 + r < L) {
            a = *reinterpret_cast<const float4 *>(Q + ((size_t)f * L + l0 + r) * ldq + h * D + q);
            if (q_colscale) {
                const float4 sc = *reinterpret_cast<const float4 *>(q_colscale + (size_t)f * H * D + h * D + q);
                a = make_float4(a.x * sc.x, a.y * sc.y, a.z * sc.z, a.w * sc.w);
            }
            a = phi4(a);
        }
        qs[r][q] = a.x, qs[r][q + 1] = a.y, qs[r][q + 2] = a.z, qs[r][q + 3] = a.w;
    }
    __syncthreads();
    const int r = t >> 2, v0 = (t & 3) * 8;
    if (l0 + r >= L) return;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float den = 0.f;
#pragma unroll 8
    for (int d = 0; d < D; ++d) {
        const float qd = qs[r][d];
        const float4 a = *reinterpret_cast<const float4 *>(&kv[d * D + v0]);
        const float4 b = *reinterpret_cast<const float4 *>(&kv[d * D + v0 + 4]);
        den = fmaf(qd, kv[D * D + d], den);
        acc[0] = fmaf(qd, a.x, acc[0]), acc[1] = fmaf(qd, a.y, acc[1]), acc[2] = fmaf(qd, a.z, acc[2]), acc[3] = fmaf(qd, a.w, acc[3]);
        acc[4] = fmaf(qd, b.x, acc[4]), acc[5] = fmaf(qd, b.y, acc[5]), acc[6] = fmaf(qd, b.z, acc[6]), acc[7] = fmaf(qd, b.w, acc[7]);
    }
    const float Z = 1.f / (den + eps), fS = (float)S;
    float *o = O + ((size_t)f * L + l0 + r) * ldo + h * D + v0;
    *reinterpret_cast<float4 *>(o) = make_float4(acc[0] * Z * fS, acc[1] * Z * fS, acc[2] * Z * fS, acc[3] * Z * fS);
    *reinterpret_cast<float4 *>(o + 4) = make_float4(acc[4] * Z * fS, acc[5] * Z * fS, acc[6] * Z * fS, acc[7] * Z * fS);
}

}  // namespace

extern "C" size_t cofi_linear_attention_workspace(int L, int S, int H, int D_, int frames) {
    if (L <= 0 || S <= 0 || H <= 0 || D_ != D || frames <= 0) return 0;
    return (size_t)frames * H * (cofi_cdiv(S, CHUNK) + 1) * SLOT * sizeof(float);
}

extern "C" int cofi_linear_attention(const float *Q, int ldq, const float *K, int ldk, const float *V, int ldv, const float *q_colscale, int L, int S,
                                     int H, int D_, float eps, int frames, float *O, int ldo, void *ws, size_t ws_bytes, cofi_stream_t stream) {
    if (!Q || !K || !V || !O || L <= 0 || S <= 0 || H <= 0 || frames <= 0) return COFI_EINVAL;
    if (D_ != D) return COFI_EUNSUPPORTED;
    if ((ldq & 3) || (ldk & 3) || (ldv & 3) || (ldo & 3) || ldq < H * D || ldk < H * D || ldv < H * D || ldo < H * D) return COFI_EINVAL;
    if (((uintptr_t)Q & 15) || ((uintptr_t)K & 15) || ((uintptr_t)V & 15) || ((uintptr_t)O & 15) || ((uintptr_t)q_colscale & 15)) return COFI_EINVAL;
    if (!ws || ((uintptr_t)ws & 15) || ws_bytes < cofi_linear_attention_workspace(L, S, H, D_, frames)) return COFI_EWORKSPACE;
    if (H > 65535 || frames > 65535 || (long)frames * H > 65535) return COFI_EUNSUPPORTED;
    const int nchunk = cofi_cdiv(S, CHUNK);
    hipStream_t st = cofi_s(stream);
    hipLaunchKernelGGL(linear_attention_summary_kernel, dim3(nchunk, H, frames), dim3(256), 0, st, K, ldk, V, ldv, S, H, nchunk, (float *)ws);
    if (int rc = cofi_launch_status()) return rc;
    hipLaunchKernelGGL(linear_attention_fold_kernel, dim3(cofi_cdiv(SLOT, 64), frames * H), dim3(256), 0, st, (float *)ws, nchunk);
    if (int rc = cofi_launch_status()) return rc;
    hipLaunchKernelGGL(linear_attention_apply_kernel, dim3(cofi_cdiv(L, TILE), H, frames), dim3(256), 0, st, Q, ldq, q_colscale, L, S, H, nchunk, eps,
                       (const float *)ws, O, ldo);
    return cofi_launch_status();
}
