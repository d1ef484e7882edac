// Registered clouds (cofi_fuse_cloud_image): the F = S * C images of a submission and its S clouds, joined through the poses the pose tail
// solved - a z-buffer per image (depth and point-id maps), per point its in-picture / visible flags in every camera, and the colour of
// the camera that sees it most centrally.  The reference has only offline numpy building blocks for this (data/kitti_helper.py:166-190
// crop_pc_with_img: np.round of K X / z, in picture when 0 <= px <= W - 1; :142-163 projection_pc_img) and no occlusion test; the contract
// is this project's (include/cofi_hip.h).
//
// Four kernels:
//   clear     every key to the all-ones sentinel and the stats to 0.  A kernel and not hipMemsetAsync: as the first node of a captured
//             graph the 0xFF memset of this range gave the right buffer on the first replay and one uniform junk key in every pixel on
//             the second (tests/test_fusion_gpu.py::test_two_runs_and_a_captured_graph_are_bit_equal); a kernel node replays as recorded.
//   zbuffer   one thread per (image, point): atomicMin of the 64-bit key (float bits of z) << 32 | point id on the (2 splat + 1)^2 pixels
//             around the point's own pixel.  z > z_near > 0, and the bit pattern of a positive float is monotone in its value, so the
//             unsigned minimum is the nearest point and, among equal depths, the lowest id.  An integer minimum does not depend on the
//             order of arrival: the buffer is bit-reproducible.
//   resolve   one thread per (cloud, point), looping over the cloud's C cameras: gate against the key of the point's own pixel, flags,
//             the most central camera, one bilinear sample there; counts reduced per workgroup, then one integer atomic per workgroup.
//   decode    one thread per pixel: key -> depth and id maps, pixels hit counted the same way.
//
// ONE projection body (project) serves zbuffer and resolve: fp32, every operation written out as a correctly rounded intrinsic (and the
// library is built with -ffp-contract=off), so a point gets bit-identical (u, v, z) in both passes and can never fail the depth test against
// its own key.  Every in-picture comparison is made on floats, before any conversion to int, in the form that a NaN fails.
#include "common.h"

namespace {

constexpr int TB = 256;

struct Cam {
    float r[9], t[3];
    float fx, fy, cx, cy;
};

struct Proj {
    float u, v, z;
    int px, py;
    bool in;
};

__device__ __forceinline__ Cam load_cam(const float *__restrict__ pose, const float *__restrict__ K, float k_scale) {
    Cam c;
#pragma unroll
    for (int i = 0; i < 9; ++i) c.r[i] = pose[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) c.t[i] = pose[9 + i];
    c.fx = __fmul_rn(K[0], k_scale);
    c.fy = __fmul_rn(K[4], k_scale);
    c.cx = __fmul_rn(K[2], k_scale);
    c.cy = __fmul_rn(K[5], k_scale);
    return c;
}

// The projection of every pass.  Row sums start from the translation and add the X, Y, Z terms in that order: three fmas per row.
__device__ __forceinline__ Proj project(const Cam &c, float X, float Y, float Z, float z_near, float wmax, float hmax) {
    Proj p;
    const float xc = __fmaf_rn(c.r[2], Z, __fmaf_rn(c.r[1], Y, __fmaf_rn(c.r[0], X, c.t[0])));
    const float yc = __fmaf_rn(c.r[5], Z, __fmaf_rn(c.r[4], Y, __fmaf_rn(c.r[3], X, c.t[1])));
    const float zc = __fmaf_rn(c.r[8], Z, __fmaf_rn(c.r[7], Y, __fmaf_rn(c.r[6], X, c.t[2])));
    p.z = zc;
    p.u = __fmaf_rn(c.fx, __fdiv_rn(xc, zc), c.cx);
    p.v = __fmaf_rn(c.fy, __fdiv_rn(yc, zc), c.cy);
    const float ru = rintf(p.u), rv = rintf(p.v);   // ties to even, as np.round
    p.in = (zc > z_near) && (ru >= 0.0f) && (ru <= wmax) && (rv >= 0.0f) && (rv <= hmax);   // a NaN fails every one
    p.px = p.in ? (int)ru : 0;
    p.py = p.in ? (int)rv : 0;
    return p;
}

// workgroup count of `flag` -> one atomicAdd by thread 0 (sh: 4 ints of LDS; two barriers)
__device__ __forceinline__ void block_count_add(bool flag, int *sh, int32_t *dst) {
    const int n = __popcll(__ballot(flag));
    __syncthreads();   // the previous use of sh is over
    if (lane_id() == 0) sh[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int total = sh[0] + sh[1] + sh[2] + sh[3];
        if (total > 0) atomicAdd(dst, total);
    }
}

__global__ __launch_bounds__(TB) void clear_kernel(unsigned long long *__restrict__ keys, unsigned n_keys, int32_t *__restrict__ stats, unsigned n_stats) {
    const unsigned i = blockIdx.x * TB + threadIdx.x;
    if (i < n_keys) keys[i] = ~0ull;
    for (unsigned j = i; j < n_stats; j += gridDim.x * TB) stats[j] = 0;
}

__global__ __launch_bounds__(TB) void zbuffer_kernel(const float *__restrict__ points, int N, int C, int H, int W,
                                                     const float *__restrict__ pose, int pose_stride, const int32_t *__restrict__ result,
                                                     int result_stride, const float *__restrict__ K, float k_scale, float z_near, int splat,
                                                     unsigned long long *__restrict__ keys) {
    const int f = blockIdx.y;
    if (result && result[(size_t)f * result_stride] == 0) return;
    const int i = blockIdx.x * TB + threadIdx.x;
    if (i >= N) return;
    const Cam cam = load_cam(pose + (size_t)f * pose_stride, K + 9 * (size_t)f, k_scale);
    const float *pt = points + 3 * ((size_t)(f / C) * N + i);
    const Proj p = project(cam, pt[0], pt[1], pt[2], z_near, (float)(W - 1), (float)(H - 1));
    if (!p.in) return;
    const unsigned long long key = ((unsigned long long)__float_as_uint(p.z) << 32) | (unsigned)i;
    unsigned long long *img = keys + (size_t)f * H * W;
    const int y0 = max(p.py - splat, 0), y1 = min(p.py + splat, H - 1), x0 = max(p.px - splat, 0), x1 = min(p.px + splat, W - 1);
    for (int y = y0; y <= y1; ++y)
        for (int x = x0; x <= x1; ++x) atomicMin(img + (size_t)y * W + x, key);
}

__global__ __launch_bounds__(TB) void resolve_kernel(const float *__restrict__ points, int N, int C, const float *__restrict__ images, int Ci,
                                                     int H, int W, const float *__restrict__ pose, int pose_stride,
                                                     const int32_t *__restrict__ result, int result_stride, const float *__restrict__ K,
                                                     float k_scale, float z_near, float rel_gain, float abs_tol,
                                                     const unsigned long long *__restrict__ keys, uint8_t *__restrict__ flags,
                                                     float *__restrict__ color, int32_t *__restrict__ camera, int32_t *__restrict__ stats) {
    __shared__ int sh[4];
    const int s = blockIdx.y;
    const int i = blockIdx.x * TB + threadIdx.x;
    const bool live = i < N;
    float X = 0.0f, Y = 0.0f, Z = 0.0f;
    if (live) {
        const float *pt = points + 3 * ((size_t)s * N + i);
        X = pt[0]; Y = pt[1]; Z = pt[2];
    }
    int best = -1;
    float best_r2 = 0.0f, best_u = 0.0f, best_v = 0.0f;
    for (int c = 0; c < C; ++c) {   // uniform over the workgroup: the barriers of block_count_add are reached by every thread
        const int f = s * C + c;
        const bool ok = !result || result[(size_t)f * result_stride] != 0;
        bool in = false, vis = false;
        if (live && ok) {
            const Cam cam = load_cam(pose + (size_t)f * pose_stride, K + 9 * (size_t)f, k_scale);
            const Proj p = project(cam, X, Y, Z, z_near, (float)(W - 1), (float)(H - 1));
            in = p.in;
            if (in) {
                const unsigned long long key = keys[((size_t)f * H + p.py) * W + p.px];
                const float zmin = __uint_as_float((unsigned)(key >> 32));
                vis = p.z <= __fmaf_rn(zmin, rel_gain, abs_tol);
                if (vis) {
                    const float du = __fdiv_rn(__fsub_rn(p.u, cam.cx), cam.fx), dv = __fdiv_rn(__fsub_rn(p.v, cam.cy), cam.fy);
                    const float r2 = __fmaf_rn(dv, dv, __fmul_rn(du, du));
                    if (best < 0 || r2 < best_r2) {   // ties keep the lower camera
                        best = c; best_r2 = r2; best_u = p.u; best_v = p.v;
                    }
                }
            }
        }
        if (live) flags[(size_t)f * N + i] = (uint8_t)((in ? 1 : 0) | (vis ? 2 : 0));
        block_count_add(in, sh, stats + 4 * f);
        block_count_add(vis, sh, stats + 4 * f + 1);
    }
    if (!live) return;
    camera[(size_t)s * N + i] = best;
    float *out = color + ((size_t)s * N + i) * Ci;
    if (best < 0) {
        for (int ch = 0; ch < Ci; ++ch) out[ch] = 0.0f;
        return;
    }
    // bilinear, pixel centres at integer coordinates, taps clamped to the edge (in picture: -0.5 <= u <= W - 0.5)
    const float fx0 = floorf(best_u), fy0 = floorf(best_v);
    const float ax = __fsub_rn(best_u, fx0), ay = __fsub_rn(best_v, fy0);
    const float wmax = (float)(W - 1), hmax = (float)(H - 1);
    const int x0 = (int)fminf(fmaxf(fx0, 0.0f), wmax), x1 = (int)fminf(fmaxf(__fadd_rn(fx0, 1.0f), 0.0f), wmax);
    const int y0 = (int)fminf(fmaxf(fy0, 0.0f), hmax), y1 = (int)fminf(fmaxf(__fadd_rn(fy0, 1.0f), 0.0f), hmax);
    const float bx = __fsub_rn(1.0f, ax), by = __fsub_rn(1.0f, ay);
    const float w00 = __fmul_rn(bx, by), w01 = __fmul_rn(ax, by), w10 = __fmul_rn(bx, ay), w11 = __fmul_rn(ax, ay);
    const float *im = images + (size_t)(s * C + best) * Ci * H * W;
    for (int ch = 0; ch < Ci; ++ch) {
        const float *pl = im + (size_t)ch * H * W;
        const float p00 = pl[(size_t)y0 * W + x0], p01 = pl[(size_t)y0 * W + x1], p10 = pl[(size_t)y1 * W + x0], p11 = pl[(size_t)y1 * W + x1];
        out[ch] = __fmaf_rn(w11, p11, __fmaf_rn(w10, p10, __fmaf_rn(w01, p01, __fmul_rn(w00, p00))));
    }
}

__global__ __launch_bounds__(TB) void decode_kernel(const unsigned long long *__restrict__ keys, int HW, float *__restrict__ depth,
                                                    int32_t *__restrict__ index, int32_t *__restrict__ stats) {
    __shared__ int sh[4];
    const int f = blockIdx.y;
    const int p = blockIdx.x * TB + threadIdx.x;
    bool hit = false;
    if (p < HW) {
        const unsigned long long key = keys[(size_t)f * HW + p];
        hit = key != ~0ull;
        depth[(size_t)f * HW + p] = hit ? __uint_as_float((unsigned)(key >> 32)) : 0.0f;
        index[(size_t)f * HW + p] = hit ? (int32_t)(unsigned)(key & 0xFFFFFFFFull) : -1;
    }
    block_count_add(hit, sh, stats + 4 * f + 2);
}

}  // namespace

extern "C" size_t cofi_fuse_workspace(int images, int H, int W) {
    if (images <= 0 || H <= 0 || W <= 0) return 0;
    const unsigned long long px = (unsigned long long)images * (unsigned long long)H * (unsigned long long)W;   // < 2^93: no wrap in 3 x 31 bits
    if ((unsigned long long)H * (unsigned long long)W > 0x7FFFFFFFull || px > 0x7FFFFFFFull) return 0;
    return (size_t)(8ull * px);
}

extern "C" int cofi_fuse_cloud_image(const float *points, int N, int images, int cameras, const float *img, int Ci, int H, int W,
                                     const float *pose, int pose_stride, const int32_t *result, int result_stride, const float *K_dev,
                                     float k_scale, float z_near, int splat, float rel_tol, float abs_tol, void *ws, size_t ws_bytes,
                                     float *depth, int32_t *index, uint8_t *flags, float *color, int32_t *camera, int32_t *stats,
                                     cofi_stream_t stream) {
    if (!points || !img || !pose || !K_dev || !ws || !depth || !index || !flags || !color || !camera || !stats) return COFI_EINVAL;
    if (N <= 0 || images <= 0 || cameras <= 0 || Ci <= 0 || H <= 0 || W <= 0 || images % cameras) return COFI_EINVAL;
    if (splat < 0 || splat > 3 || pose_stride < 12 || (result && result_stride < 1)) return COFI_EINVAL;
    if (!(z_near > 0.0f) || !(rel_tol >= 0.0f) || !(abs_tol >= 0.0f) || !(k_scale > 0.0f)) return COFI_EINVAL;   // keys order positive depths only
    const size_t need = cofi_fuse_workspace(images, H, W);   // 0: images * H * W beyond 31 bits
    if (need == 0) return COFI_EINVAL;
    if (ws_bytes < need) return COFI_EWORKSPACE;
    if (((uintptr_t)ws & 7) != 0) return COFI_EINVAL;
    if (images > 65535) return COFI_EUNSUPPORTED;   // the image / cloud is the grid's second axis
    const int S = images / cameras, HW = H * W;
    unsigned long long *keys = (unsigned long long *)ws;
    hipLaunchKernelGGL(clear_kernel, dim3(cofi_cdiv((long)images * HW, TB)), dim3(TB), 0, cofi_s(stream), keys, (unsigned)(images * HW), stats,
                       (unsigned)(4 * images));
    hipLaunchKernelGGL(zbuffer_kernel, dim3(cofi_cdiv(N, TB), images), dim3(TB), 0, cofi_s(stream), points, N, cameras, H, W, pose, pose_stride,
                       result, result_stride, K_dev, k_scale, z_near, splat, keys);
    hipLaunchKernelGGL(resolve_kernel, dim3(cofi_cdiv(N, TB), S), dim3(TB), 0, cofi_s(stream), points, N, cameras, img, Ci, H, W, pose,
                       pose_stride, result, result_stride, K_dev, k_scale, z_near, 1.0f + rel_tol, abs_tol, keys, flags, color, camera, stats);
    hipLaunchKernelGGL(decode_kernel, dim3(cofi_cdiv(HW, TB), images), dim3(TB), 0, cofi_s(stream), keys, HW, depth, index, stats);
    return cofi_launch_status();
}
