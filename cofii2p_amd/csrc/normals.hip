// Surface normals of a raw scan from its k-nearest rows (cofi_estimate_normals): per point the unit eigenvector of the smallest
// eigenvalue of the covariance of its neighbourhood, oriented towards a viewpoint.  The reference reads this normal from disk
// (data/kitti.py:130, pc_npy_with_normal) and computes it nowhere; the contract is this project's (include/cofi_hip.h).
//
// Layout: 16 lanes per query, 4 queries per wave, 16 per workgroup of 256.  The lanes of a group stride over the row's slots - index
// and distance reads are contiguous per group - and each lane gathers its points; the nine sums and the slot count go through an xor
// butterfly inside the group (no LDS, no atomics), after which every lane of the group holds the same sums and runs the 3 x 3 solve
// redundantly: the wave stays convergent and no broadcast is needed.  Lanes 0..2 of a group write one component each.
//
// Numerics (fp32 throughout): d = neighbour - query first (coordinates reach +-80 m, a neighbourhood spans decimetres), sum d and the
// six unique sum d d^T, C = sum d d^T / m - (sum d / m)(sum d / m)^T, scaled by a power of two (exact) to trace in [1/2, 1).  Five cyclic
// Jacobi sweeps (branch-free: a zero off-diagonal entry selects the identity rotation, so lambda0 = 0 exactly is no special case) give
// eigenvalues and vectors to a few ulp; one first-order correction of the chosen vector against the UNROTATED matrix,
//     n <- n - sum_j v_j (v_j^T A n) / (lambda_j - lambda_0),
// removes what the fifteen rotations accumulated in it (skipped for a partner eigenvalue within 16 ulp of lambda_0, where the direction
// inside the shared eigenspace is free anyway).  The sign is a function of the input alone: largest component positive (lowest axis on
// ties), then flipped when it points away from the viewpoint.
#include "common.h"

namespace {

constexpr int NG = 16;                 // lanes per query
constexpr int NQ_WG = 256 / NG;        // queries per workgroup
constexpr int JACOBI_SWEEPS = 5;

struct V3 {
    float x, y, z;
};

// One Jacobi rotation in the (p, q) plane of a symmetric 3 x 3 matrix, r = the third index: zeroes a_pq, updates the two diagonal
// entries, the two remaining off-diagonal entries and the eigenvector columns p and q.
__device__ __forceinline__ void jacobi_rotate(float &app, float &aqq, float &apq, float &arp, float &arq, V3 &vp, V3 &vq) {
    const float theta = (aqq - app) / (2.0f * apq);
    float t = copysignf(1.0f, theta) / (fabsf(theta) + sqrtf(theta * theta + 1.0f));   // theta = +-inf (or its square): t = 0
    t = apq == 0.0f ? 0.0f : t;                                                         // 0 / 0 above: identity rotation
    const float c = 1.0f / sqrtf(t * t + 1.0f), s = t * c;
    app -= t * apq;
    aqq += t * apq;
    apq = 0.0f;
    const float rp = c * arp - s * arq, rq = s * arp + c * arq;
    arp = rp;
    arq = rq;
    const V3 np = {c * vp.x - s * vq.x, c * vp.y - s * vq.y, c * vp.z - s * vq.z};
    const V3 nq = {s * vp.x + c * vq.x, s * vp.y + c * vq.y, s * vp.z + c * vq.z};
    vp = np;
    vq = nq;
}

__device__ __forceinline__ float dot3(const V3 &a, const V3 &b) { return a.x * b.x + a.y * b.y + a.z * b.z; }

__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
    for (int o = NG / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(256) void estimate_normals_kernel(const float *__restrict__ points, int S, const int32_t *__restrict__ idx,
                                                               const float *__restrict__ dist, int Q, int k, int ldi, float r2,
                                                               const float *__restrict__ viewpoint, float *__restrict__ out,
                                                               long long out_point_stride, long long out_comp_stride,
                                                               int32_t *__restrict__ degenerate_count) {
    const int sub = threadIdx.x & (NG - 1);
    const int q_raw = blockIdx.x * NQ_WG + (threadIdx.x / NG);
    const bool live = q_raw < Q;
    const int q = live ? q_raw : Q - 1;   // tail groups redo the last query (every lane stays in the shuffles), they write and count nothing
    const float px = points[3 * (size_t)q], py = points[3 * (size_t)q + 1], pz = points[3 * (size_t)q + 2];

    float sx = 0.f, sy = 0.f, sz = 0.f, sxx = 0.f, syy = 0.f, szz = 0.f, sxy = 0.f, sxz = 0.f, syz = 0.f, cnt = 0.f;
    const size_t row = (size_t)q * (size_t)ldi;
    for (int j = sub; j < k; j += NG) {
        const int id = idx[row + j];
        bool keep = (unsigned)id < (unsigned)S;          // the search pads with the shadow index S when S < k
        if (r2 >= 0.0f) keep = keep && dist[row + j] <= r2;
        if (keep) {
            const float dx = points[3 * (size_t)id] - px, dy = points[3 * (size_t)id + 1] - py, dz = points[3 * (size_t)id + 2] - pz;
            sx += dx; sy += dy; sz += dz;
            sxx += dx * dx; syy += dy * dy; szz += dz * dz;
            sxy += dx * dy; sxz += dx * dz; syz += dy * dz;
            cnt += 1.0f;
        }
    }
    sx = group_sum(sx); sy = group_sum(sy); sz = group_sum(sz);
    sxx = group_sum(sxx); syy = group_sum(syy); szz = group_sum(szz);
    sxy = group_sum(sxy); sxz = group_sum(sxz); syz = group_sum(syz);
    const float m = group_sum(cnt);                      // <= 128: exact

    const float mdiv = fmaxf(m, 1.0f);
    const float mx = sx / mdiv, my = sy / mdiv, mz = sz / mdiv;
    float a00 = sxx / mdiv - mx * mx, a11 = syy / mdiv - my * my, a22 = szz / mdiv - mz * mz;
    float a01 = sxy / mdiv - mx * my, a02 = sxz / mdiv - mx * mz, a12 = syz / mdiv - my * mz;
    const float tr = a00 + a11 + a22;
    bool degenerate = m < 3.0f || !(tr > 0.0f);          // also a NaN trace
    {   // exact scaling to trace in [1/2, 1); a denormal trace below 2^-128 overflows the scale to inf: the row then fails the finiteness
        // test below and is degenerate, as neighbours that coincide to within fp32's range should be
        const float sc = ldexpf(1.0f, -(ilogbf(degenerate ? 1.0f : tr) + 1));
        a00 *= sc; a11 *= sc; a22 *= sc; a01 *= sc; a02 *= sc; a12 *= sc;
    }
    const float b00 = a00, b11 = a11, b22 = a22, b01 = a01, b02 = a02, b12 = a12;

    V3 v0 = {1.f, 0.f, 0.f}, v1 = {0.f, 1.f, 0.f}, v2 = {0.f, 0.f, 1.f};
#pragma unroll
    for (int sweep = 0; sweep < JACOBI_SWEEPS; ++sweep) {
        jacobi_rotate(a00, a11, a01, a02, a12, v0, v1);
        jacobi_rotate(a00, a22, a02, a01, a12, v0, v2);
        jacobi_rotate(a11, a22, a12, a01, a02, v1, v2);
    }
    // smallest eigenvalue (lowest index on ties) and its two partners
    const int i0 = (a00 <= a11 && a00 <= a22) ? 0 : (a11 <= a22 ? 1 : 2);
    const float l0 = i0 == 0 ? a00 : (i0 == 1 ? a11 : a22);
    V3 n = i0 == 0 ? v0 : (i0 == 1 ? v1 : v2);
    const V3 va = i0 == 0 ? v1 : v0, vb = i0 == 2 ? v1 : v2;
    const float da = (i0 == 0 ? a11 : a00) - l0, db = (i0 == 2 ? a11 : a22) - l0;
    {
        const V3 An = {b00 * n.x + b01 * n.y + b02 * n.z, b01 * n.x + b11 * n.y + b12 * n.z, b02 * n.x + b12 * n.y + b22 * n.z};
        const float tiny = 9.5367431640625e-7f;   // 16 * 2^-24 of the trace
        const float ca = da > tiny ? dot3(va, An) / da : 0.0f, cb = db > tiny ? dot3(vb, An) / db : 0.0f;
        n.x -= ca * va.x + cb * vb.x;
        n.y -= ca * va.y + cb * vb.y;
        n.z -= ca * va.z + cb * vb.z;
    }
    const float inv = 1.0f / sqrtf(dot3(n, n));
    n.x *= inv; n.y *= inv; n.z *= inv;
    const float ax = fabsf(n.x), ay = fabsf(n.y), az = fabsf(n.z);
    degenerate = degenerate || !(ax + ay + az < INFINITY);   // NaN / inf

    // sign: the component of largest magnitude positive (lowest axis on ties), then towards the viewpoint
    const float lead = (ax >= ay && ax >= az) ? n.x : (ay >= az ? n.y : n.z);
    bool flip = lead < 0.0f;
    if (viewpoint) {
        const float s = (flip ? -1.0f : 1.0f) * (n.x * (viewpoint[0] - px) + n.y * (viewpoint[1] - py) + n.z * (viewpoint[2] - pz));
        flip = flip != (s < 0.0f);
    }
    if (flip) { n.x = -n.x; n.y = -n.y; n.z = -n.z; }
    if (degenerate) { n.x = 0.0f; n.y = 0.0f; n.z = 1.0f; }

    if (live && sub < 3)
        out[(long long)q * out_point_stride + (long long)sub * out_comp_stride] = sub == 0 ? n.x : (sub == 1 ? n.y : n.z);
    if (degenerate_count) {   // one atomic per wave at most
        const int nd = __popcll(__ballot(live && sub == 0 && degenerate));
        if ((threadIdx.x & 63) == 0 && nd > 0) atomicAdd(degenerate_count, nd);
    }
}

}  // namespace

extern "C" int cofi_estimate_normals(const float *points, int S, const int32_t *idx, const float *dist, int Q, int k, int ldi, float radius,
                                     const float *viewpoint3_dev, float *out, long long out_point_stride, long long out_comp_stride,
                                     int32_t *degenerate_count_dev, cofi_stream_t stream) {
    if (!points || !idx || !out || S <= 0 || Q < 0 || Q > S || k <= 0 || k > 128 || ldi < k) return COFI_EINVAL;
    if (radius > 0.0f && !dist) return COFI_EINVAL;
    if (out_point_stride == 0 || out_comp_stride == 0) return COFI_EINVAL;
    if (Q == 0) return 0;
    hipLaunchKernelGGL(estimate_normals_kernel, dim3(cofi_cdiv(Q, NQ_WG)), dim3(256), 0, cofi_s(stream), points, S, idx, dist, Q, k, ldi,
                       radius > 0.0f ? radius * radius : -1.0f, viewpoint3_dev, out, out_point_stride, out_comp_stride, degenerate_count_dev);
    return cofi_launch_status();
}
