// ABI identification of libcofi_hip.so.
#include "common.h"

extern "C" int cofi_abi_version(void) { return COFI_ABI_VERSION; }
extern "C" const char *cofi_target_arch(void) { return "gfx950"; }

// Batched device-to-device copy: ONE launch moves a whole list of tensors (the per-frame inputs into the static buffers a
// captured hipGraph reads).  20+ separate copies cost ~3 us of stream time each; the descriptors travel as one small H2D copy.
namespace {
struct CopyDesc {
    const void *src;
    void *dst;
    unsigned long long bytes;
};

__global__ __launch_bounds__(256) void multi_copy_kernel(const CopyDesc *descs) {
    const CopyDesc d = descs[blockIdx.y];
    const size_t n16 = (((uintptr_t)d.src | (uintptr_t)d.dst) & 15) ? 0 : d.bytes / 16;
    const uint4 *s4 = reinterpret_cast<const uint4 *>(d.src);
    uint4 *d4 = reinterpret_cast<uint4 *>(d.dst);
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    // four independent 16-byte loads in flight per lane: the 10 MB neighbour table of a frame is latency-bound otherwise
    for (; i + 3 * stride < n16; i += 4 * stride) {
        const uint4 v0 = s4[i], v1 = s4[i + stride], v2 = s4[i + 2 * stride], v3 = s4[i + 3 * stride];
        d4[i] = v0; d4[i + stride] = v1; d4[i + 2 * stride] = v2; d4[i + 3 * stride] = v3;
    }
    for (; i < n16; i += stride) d4[i] = s4[i];
    const unsigned char *sb = reinterpret_cast<const unsigned char *>(d.src);
    unsigned char *db = reinterpret_cast<unsigned char *>(d.dst);
    for (size_t b = n16 * 16 + (size_t)blockIdx.x * blockDim.x + threadIdx.x; b < d.bytes; b += stride) db[b] = sb[b];
}

// dst row (s * times + c) * rows + r <- src row s * rows + r for every c < times: each source unit is read once and stored `times`
// times.  A row is v4 16-byte units followed by cols - 4 * v4 single floats (v4 = 0 when a pointer or a leading dimension is not
// 16-byte aligned); columns >= cols of dst are not touched.
__global__ __launch_bounds__(256) void repeat_frames_kernel(const float *src, int lds, int rows, int cols, size_t src_rows, int times,
                                                            float *dst, int ldd, int v4) {
    const int units = v4 + (cols - 4 * v4);
    const size_t total = src_rows * units, stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const size_t row = i / units;
        const int u = (int)(i - row * units);
        const size_t s = row / rows, r = row - s * rows;
        const float *sp = src + row * lds;
        float *dp = dst + (s * times * rows + r) * ldd;
        if (u < v4) {
            const uint4 v = reinterpret_cast<const uint4 *>(sp)[u];
            for (int c = 0; c < times; ++c) reinterpret_cast<uint4 *>(dp + (size_t)c * rows * ldd)[u] = v;
        } else {
            const int col = 4 * v4 + (u - v4);
            const float v = sp[col];
            for (int c = 0; c < times; ++c) dp[(size_t)c * rows * ldd + col] = v;
        }
    }
}
}  // namespace

extern "C" int cofi_repeat_frames(const float *src, int lds, int rows_per_frame, int cols, int frames, int times, float *dst, int ldd,
                                  cofi_stream_t stream) {
    if (!src || !dst || rows_per_frame <= 0 || cols <= 0 || frames <= 0 || times <= 0 || lds < cols || ldd < cols) return COFI_EINVAL;
    const bool aligned = !((((uintptr_t)src | (uintptr_t)dst) & 15) || (lds & 3) || (ldd & 3));
    const int v4 = aligned ? cols / 4 : 0;
    const size_t src_rows = (size_t)frames * rows_per_frame, total = src_rows * (size_t)(v4 + cols - 4 * v4);
    const size_t blocks = (total + 255) / 256;
    hipLaunchKernelGGL(repeat_frames_kernel, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0, cofi_s(stream), src, lds,
                       rows_per_frame, cols, src_rows, times, dst, ldd, v4);
    return cofi_launch_status();
}

extern "C" int cofi_multi_copy(const void *descs_dev, int n, int blocks_per_copy, cofi_stream_t stream) {
    if (!descs_dev || n < 0 || blocks_per_copy <= 0) return COFI_EINVAL;
    if (n == 0) return 0;
    hipLaunchKernelGGL(multi_copy_kernel, dim3(blocks_per_copy, n), dim3(256), 0, cofi_s(stream), (const CopyDesc *)descs_dev);
    return cofi_launch_status();
}
