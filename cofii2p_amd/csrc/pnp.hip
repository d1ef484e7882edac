// Camera pose from the fine 2-D / 3-D matches: RANSAC over P3P hypotheses + Levenberg-Marquardt refit, all on the device.
// Replaces the pose step of the reference's evaluation (evaluation/eval_all.py:107):
//     cv2.solvePnPRansac(cameraMatrix=K, imagePoints=fine_xy.T, objectPoints=coarse_pc_points, iterationsCount=10000, distCoeffs=None)
// i.e. reprojection threshold 8 px, minimal-set hypotheses, best consensus set, iterative (LM) refit on its inliers.  OpenCV is a
// third-party dependency that is absent here: parity with it is UNPINNED; the restatement this kernel is checked against is
// oracle/pnp_oracle.py (same counter-based samples, same algorithm), which is validated geometrically.
//
// Kernel 1: one wave per HPW = 16 hypotheses.  Lane h < 16 draws 4 correspondences, solves P3P (Grunert: the depth ratios
//   satisfy a quartic whose coefficients come from polynomial arithmetic; closed-form Ferrari roots polished by Newton, fp64) on
//   three of them and lets the fourth choose among the up-to-four poses.  Then the wave scores its 16 poses one after the other,
//   lanes striding over the correspondences (fp32), and publishes (inliers << 32 | ~hypothesis) with an integer atomicMax:
//   the winner is the hypothesis with most inliers, lowest id on ties - deterministic.
// Kernel 2: one workgroup refits the winner on its inliers: LM on the reprojection error with left-multiplied se(3) increments,
//   normal equations reduced in a fixed order (fp64), 6x6 solve by one thread.
// Both kernels exist in two forms around ONE body each (hypotheses_wave, refine_workgroup): per frame (cofi_pnp_ransac), and batched
//   (cofi_pnp_ransac_batch: frame on the grid, operands addressed through strides, count and intrinsics read on the device; a workgroup
//   of 4 waves stages its frame's correspondences once in LDS and its 64 hypotheses score from there).  The bodies receive VALUES through
//   an accessor, so frame f of a batch executes the arithmetic of the per-frame call in the same order: bit-identical results.
// A third form, the rig (cofi_pnp_ransac_rig): C images of one body, ONE pose.  The bodies take a VIEW that answers how many cameras there
//   are, how a hypothesis is solved and what each camera scores; a frame of its own is the view with one camera whose compositions are
//   copies, so the per-frame and batched kernels compute what they always did.  A rig hypothesis is a P3P solve in ONE camera (drawn in
//   proportion to the cameras' rows) carried into the rig frame through that camera's extrinsics; it is scored and refitted over ALL cameras.
// Kernel 3 (pose_errors_kernel): RTE / RRE of B poses against ground truth, one thread per frame, fp64.
// Kernel 4 (covariance_body behind cofi_pose_covariance, _batch, _rig): the 6x6 covariance and information matrix of a returned pose from
//   the refit's own normal equations over the consensus set, one wave per body; pose_nees_kernel scores it against ground truth.
#include <type_traits>

#include "common.h"
#include "pose_errors.h"

namespace {

constexpr int HPW = 16;  // hypotheses per wave

__device__ __forceinline__ unsigned hash_u32(unsigned seed, unsigned hyp, unsigned j) {
    unsigned x = seed * 0x9E3779B1u + hyp * 0x85EBCA77u + j * 0xC2B2AE3Du + 0x27D4EB2Fu;
    x ^= x >> 16; x *= 0x7FEB352Du;
    x ^= x >> 15; x *= 0x846CA68Bu;
    x ^= x >> 16;
    return x;
}

struct Cam { float fx, fy, cx, cy; };

// real roots of q0 + q1 x + ... + q4 x^4 (q4 != 0): Ferrari, then Newton on the original quartic
__device__ int quartic_real_roots(const double q[5], double out[4]) {
    const double a = q[3] / q[4], b = q[2] / q[4], c = q[1] / q[4], d = q[0] / q[4];
    const double a2 = a * a;
    const double p = b - 0.375 * a2, qq = c - 0.5 * a * b + 0.125 * a2 * a, r = d - 0.25 * a * c + 0.0625 * a2 * b - 0.01171875 * a2 * a2;
    double y[4];
    int n = 0;
    const double scale = fabs(p) + fabs(r) + 1.0;
    if (fabs(qq) < 1e-12 * scale) {  // biquadratic
        const double disc = p * p - 4.0 * r;
        if (disc >= 0.0) {
            const double sd = sqrt(disc);
            const double z1 = 0.5 * (-p + sd), z2 = 0.5 * (-p - sd);
            if (z1 >= 0.0) { y[n++] = sqrt(z1); y[n++] = -sqrt(z1); }
            if (z2 >= 0.0) { y[n++] = sqrt(z2); y[n++] = -sqrt(z2); }
        }
    } else {
        // resolvent cubic m^3 + p m^2 + (p^2/4 - r) m - q^2/8 = 0: largest real root (positive because q != 0)
        const double c2 = p, c1 = 0.25 * p * p - r, c0 = -0.125 * qq * qq;
        const double P = c1 - c2 * c2 / 3.0, Q = 2.0 * c2 * c2 * c2 / 27.0 - c2 * c1 / 3.0 + c0;
        const double disc = 0.25 * Q * Q + P * P * P / 27.0;
        double t;
        if (disc >= 0.0) {
            const double sd = sqrt(disc);
            t = cbrt(-0.5 * Q + sd) + cbrt(-0.5 * Q - sd);
        } else {
            const double rr = sqrt(-P / 3.0);
            double arg = 1.5 * Q / (P * rr);
            arg = arg > 1.0 ? 1.0 : (arg < -1.0 ? -1.0 : arg);
            t = 2.0 * rr * cos(acos(arg) / 3.0);
        }
        double m = t - c2 / 3.0;
        for (int it = 0; it < 3; ++it) {  // polish the cubic root
            const double f = ((m + c2) * m + c1) * m + c0, df = (3.0 * m + 2.0 * c2) * m + c1;
            if (df != 0.0) m -= f / df;
        }
        if (m > 0.0) {
            const double s = sqrt(2.0 * m), h = 0.5 * p + m, g = qq / (2.0 * s);
            const double d1 = s * s - 4.0 * (h + g), d2 = s * s - 4.0 * (h - g);
            if (d1 >= 0.0) { const double sd = sqrt(d1); y[n++] = 0.5 * (s + sd); y[n++] = 0.5 * (s - sd); }
            if (d2 >= 0.0) { const double sd = sqrt(d2); y[n++] = 0.5 * (-s + sd); y[n++] = 0.5 * (-s - sd); }
        }
    }
    for (int i = 0; i < n; ++i) {
        double x = y[i] - 0.25 * a;
        for (int it = 0; it < 3; ++it) {
            const double f = (((q[4] * x + q[3]) * x + q[2]) * x + q[1]) * x + q[0];
            const double df = ((4.0 * q[4] * x + 3.0 * q[3]) * x + 2.0 * q[2]) * x + q[1];
            if (df != 0.0) x -= f / df;
        }
        out[i] = x;
    }
    return n;
}

__device__ __forceinline__ void cross3(const double a[3], const double b[3], double o[3]) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}

// orthonormal frame of a triangle: columns e1 = (A1-A0)/|.|, e2 = e3 x e1, e3 = e1 x (A2-A0) / |.|
__device__ bool tri_frame(const double A[3][3], double F[3][3]) {
    double e1[3] = {A[1][0] - A[0][0], A[1][1] - A[0][1], A[1][2] - A[0][2]};
    double w[3] = {A[2][0] - A[0][0], A[2][1] - A[0][1], A[2][2] - A[0][2]};
    const double n1 = sqrt(e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2]);
    double e3[3];
    cross3(e1, w, e3);
    const double n3 = sqrt(e3[0] * e3[0] + e3[1] * e3[1] + e3[2] * e3[2]);
    if (n1 < 1e-12 || n3 < 1e-12) return false;
    for (int i = 0; i < 3; ++i) { e1[i] /= n1; e3[i] /= n3; }
    double e2[3];
    cross3(e3, e1, e2);
    for (int i = 0; i < 3; ++i) { F[i][0] = e1[i]; F[i][1] = e2[i]; F[i][2] = e3[i]; }
    return true;
}

// P3P on (X[0..2], bearing f[0..2]); the 4th correspondence (X4, uv4) picks the pose.  pose = R row-major (9) | t (3)
__device__ bool p3p_pick(const double X[3][3], const double f[3][3], const double X4[3], double u4, double v4, const Cam &cam,
                         double pose[12]) {
    auto d2 = [&](int i, int j) {
        const double x = X[i][0] - X[j][0], y = X[i][1] - X[j][1], z = X[i][2] - X[j][2];
        return x * x + y * y + z * z;
    };
    const double a2 = d2(1, 2), b2 = d2(0, 2), c2 = d2(0, 1);
    if (fmin(a2, fmin(b2, c2)) < 1e-18) return false;
    auto dot = [&](int i, int j) { return f[i][0] * f[j][0] + f[i][1] * f[j][1] + f[i][2] * f[j][2]; };
    const double ca = dot(1, 2), cb = dot(0, 2), cg = dot(0, 1);
    // polynomials in v = s3/s1, lowest degree first (see oracle/pnp_oracle.py::p3p_grunert)
    const double w[3] = {1.0, -2.0 * cb, 1.0};
    const double N[3] = {(a2 - c2) * w[0] + b2, (a2 - c2) * w[1], (a2 - c2) * w[2] - b2};
    const double D[2] = {2.0 * b2 * cg, -2.0 * b2 * ca};
    const double D2[3] = {D[0] * D[0], 2.0 * D[0] * D[1], D[1] * D[1]};
    double N2[5] = {0, 0, 0, 0, 0}, ND[4] = {0, 0, 0, 0}, WD2[5] = {0, 0, 0, 0, 0};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) { N2[i + j] += N[i] * N[j]; WD2[i + j] += w[i] * D2[j]; }
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 2; ++j) ND[i + j] += N[i] * D[j];
    double q[5];
    for (int k = 0; k < 5; ++k) q[k] = b2 * ((k < 3 ? D2[k] : 0.0) + N2[k] - 2.0 * cg * (k < 4 ? ND[k] : 0.0)) - c2 * WD2[k];
    const double qs = fabs(q[0]) + fabs(q[1]) + fabs(q[2]) + fabs(q[3]) + fabs(q[4]);
    if (!(fabs(q[4]) > 1e-14 * qs)) return false;
    double roots[4];
    const int nr = quartic_real_roots(q, roots);
    double best = 1e300;
    bool found = false;
    for (int i = 0; i < nr; ++i) {
        const double v = roots[i];
        const double den = D[0] + D[1] * v;
        if (!(v > 0.0) || fabs(den) < 1e-12) continue;
        const double u = (N[0] + N[1] * v + N[2] * v * v) / den;
        const double wv = 1.0 - 2.0 * v * cb + v * v;
        if (!(u > 0.0) || !(wv > 0.0)) continue;
        const double s1 = sqrt(b2 / wv), s[3] = {s1, u * s1, v * s1};
        double C[3][3], Fp[3][3], Fc[3][3];
        for (int k = 0; k < 3; ++k)
            for (int e = 0; e < 3; ++e) C[k][e] = s[k] * f[k][e];
        if (!tri_frame(X, Fp) || !tri_frame(C, Fc)) continue;
        double R[9], t[3];
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) R[3 * r + c] = Fc[r][0] * Fp[c][0] + Fc[r][1] * Fp[c][1] + Fc[r][2] * Fp[c][2];
        for (int r = 0; r < 3; ++r) t[r] = C[0][r] - (R[3 * r] * X[0][0] + R[3 * r + 1] * X[0][1] + R[3 * r + 2] * X[0][2]);
        // reprojection of the 4th correspondence
        const double y0 = R[0] * X4[0] + R[1] * X4[1] + R[2] * X4[2] + t[0], y1 = R[3] * X4[0] + R[4] * X4[1] + R[5] * X4[2] + t[1],
                     y2 = R[6] * X4[0] + R[7] * X4[1] + R[8] * X4[2] + t[2];
        if (!(y2 > 1e-6)) continue;
        const double eu = cam.fx * y0 / y2 + cam.cx - u4, ev = cam.fy * y1 / y2 + cam.cy - v4;
        const double e = eu * eu + ev * ev;
        if (e < best) {
            best = e;
            found = true;
            for (int k = 0; k < 9; ++k) pose[k] = R[k];
            for (int k = 0; k < 3; ++k) pose[9 + k] = t[k];
        }
    }
    return found;
}

__device__ __forceinline__ bool inlier(const float p[12], const float *X, const float *uv, const Cam &cam, float thr2) {
    const float y0 = p[0] * X[0] + p[1] * X[1] + p[2] * X[2] + p[9], y1 = p[3] * X[0] + p[4] * X[1] + p[5] * X[2] + p[10],
                y2 = p[6] * X[0] + p[7] * X[1] + p[8] * X[2] + p[11];
    const float eu = cam.fx * y0 / y2 + cam.cx - uv[0], ev = cam.fy * y1 / y2 + cam.cy - uv[1];
    return y2 > 1e-6f && eu * eu + ev * ev <= thr2;
}

// Where a kernel finds correspondence i.  Every kernel below takes one of these and hands VALUES (X[3], uv[2]) to the shared device
// functions, so the per-frame and the batched kernels execute the same arithmetic whatever the operand layout.
struct CorrGlobal {   // global memory: object point i at obj[3 i ..], pixel i at (u[i * step], v[i * step])
    const float *obj, *u, *v;
    int step;         // 2: point-major (n, 2) with v = u + 1;  1: coordinate-major (2, n) with v = u + n_max
    __device__ __forceinline__ void load(int i, float X[3], float uv[2]) const {
        X[0] = obj[3 * i]; X[1] = obj[3 * i + 1]; X[2] = obj[3 * i + 2];
        uv[0] = u[(size_t)i * step]; uv[1] = v[(size_t)i * step];
    }
};
struct CorrLds {      // structure of arrays in LDS, `ld` floats apart: x | y | z | u | v (20 bytes per correspondence, conflict-free strides)
    const float *s;
    int ld;
    __device__ __forceinline__ void load(int i, float X[3], float uv[2]) const {
        X[0] = s[i]; X[1] = s[ld + i]; X[2] = s[2 * ld + i];
        uv[0] = s[3 * ld + i]; uv[1] = s[4 * ld + i];
    }
};

// The minimal solve of hypothesis `hyp` among n correspondences of one camera: four distinct rows, P3P on three, the fourth picks.
// pose (fp64, not yet rounded) = that camera <- cloud.
template <class Corr>
__device__ __forceinline__ bool solve_minimal(const Corr &corr, int n, const Cam &cam, unsigned seed, int hyp, double pose[12]) {
    int idx[4];
    for (int j = 0; j < 4; ++j) {
        int c = (int)(hash_u32(seed, (unsigned)hyp, (unsigned)j) % (unsigned)n);
        bool again = true;
        while (again) {
            again = false;
            for (int k = 0; k < j; ++k)
                if (idx[k] == c) { c = (c + 1) % n; again = true; }
        }
        idx[j] = c;
    }
    double X[3][3], f[3][3];
    float Xf[3], uvf[2];
    for (int k = 0; k < 3; ++k) {
        corr.load(idx[k], Xf, uvf);
        for (int e = 0; e < 3; ++e) X[k][e] = (double)Xf[e];
        const double bx = ((double)uvf[0] - cam.cx) / cam.fx, by = ((double)uvf[1] - cam.cy) / cam.fy;
        const double inv = 1.0 / sqrt(bx * bx + by * by + 1.0);
        f[k][0] = bx * inv; f[k][1] = by * inv; f[k][2] = inv;
    }
    corr.load(idx[3], Xf, uvf);
    const double X4[3] = {(double)Xf[0], (double)Xf[1], (double)Xf[2]};
    return p3p_pick(X, f, X4, (double)uvf[0], (double)uvf[1], cam, pose);
}

// Rig extrinsics, 12 floats per camera [R row-major | t], camera <- rig: Y_cam = R_c Y_rig + t_c.  Everything is composed in fp64 and
// rounded once by the caller.  With the identity both compositions multiply by 1 and add 0: exact.
__device__ __forceinline__ void ext_compose(const float *e, const double T[12], double P[12]) {       // P = E o T
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) P[3 * r + c] = (double)e[3 * r] * T[c] + (double)e[3 * r + 1] * T[3 + c] + (double)e[3 * r + 2] * T[6 + c];
        P[9 + r] = (double)e[3 * r] * T[9] + (double)e[3 * r + 1] * T[10] + (double)e[3 * r + 2] * T[11] + (double)e[9 + r];
    }
}
__device__ __forceinline__ void ext_compose_inverse(const float *e, const double P[12], double T[12]) {   // T = E^-1 o P
    const double d[3] = {P[9] - (double)e[9], P[10] - (double)e[10], P[11] - (double)e[11]};
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) T[3 * r + c] = (double)e[r] * P[c] + (double)e[3 + r] * P[3 + c] + (double)e[6 + r] * P[6 + c];
        T[9 + r] = (double)e[r] * d[0] + (double)e[3 + r] * d[1] + (double)e[6 + r] * d[2];
    }
}

// What the hypotheses body works on.  A view answers: how many cameras, the minimal solve of a hypothesis (pose of the BODY: the camera
// of a single frame, the rig of a rig), and per camera what to score (correspondences, intrinsics, the body pose carried into that camera).
template <class Corr>
struct OneCameraView {      // a frame of its own: per-frame and batched kernels
    Corr corr_;
    int n;
    Cam cam_;
    struct Scored {
        Corr corr;
        int n;
        Cam cam;
        bool scored;
        __device__ __forceinline__ void carry(const float T[12], float p[12]) const {
            for (int k = 0; k < 12; ++k) p[k] = T[k];
        }
    };
    __device__ __forceinline__ int cameras() const { return 1; }
    __device__ __forceinline__ bool solve(unsigned seed, int hyp, double pose[12]) const { return solve_minimal(corr_, n, cam_, seed, hyp, pose); }
    __device__ __forceinline__ Scored score_camera(int) const { return Scored{corr_, n, cam_, true}; }
};

// One wave, HPW hypotheses hyp0 .. hyp0 + HPW - 1 (lane h < HPW solves hypothesis hyp0 + h, then all 64 lanes score the HPW poses one
// after the other, camera by camera; lane h keeps the inlier count of hypothesis hyp0 + h).  The body of all hypotheses kernels.
template <class View>
__device__ __forceinline__ void hypotheses_wave(const View &view, int iters, float thr2, unsigned seed, int hyp0, float *poses,
                                                unsigned long long *best_key) {
    const int lane = threadIdx.x & 63;
    const int hyp = hyp0 + lane;
    float pose_f[12];
    bool ok = false;
    if (lane < HPW && hyp < iters) {
        double pose[12];
        ok = view.solve(seed, hyp, pose);
        if (ok)
            for (int k = 0; k < 12; ++k) {
                pose_f[k] = (float)pose[k];
                poses[(size_t)hyp * 12 + k] = pose_f[k];
            }
    }
    // score the wave's hypotheses one after the other: lanes stride over the correspondences
    int mine = 0;
    for (int c = 0; c < view.cameras(); ++c) {
        const auto sc = view.score_camera(c);   // workgroup-uniform (a view that stages rows has its barriers in here)
        if (!sc.scored) continue;
        float carried[12];
        if (ok) sc.carry(pose_f, carried);
        for (int h = 0; h < HPW; ++h) {
            if (!__shfl((int)ok, h, 64)) continue;   // uniform
            float p[12];
#pragma unroll
            for (int k = 0; k < 12; ++k) p[k] = __shfl(carried[k], h, 64);
            int cnt = 0;
            for (int i = lane; i < sc.n; i += 64) {
                float Xi[3], uvi[2];
                sc.corr.load(i, Xi, uvi);
                cnt += inlier(p, Xi, uvi, sc.cam, thr2) ? 1 : 0;
            }
            for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
            mine += lane == h ? cnt : 0;
        }
    }
    unsigned long long wave_best = ok ? ((unsigned long long)(unsigned)mine << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)hyp) : 0ull;
    for (int o = HPW / 2; o > 0; o >>= 1) {   // lanes >= HPW hold 0
        const unsigned long long other = __shfl_xor(wave_best, o, 64);
        wave_best = other > wave_best ? other : wave_best;
    }
    if (lane == 0 && wave_best) atomicMax(best_key, wave_best);
}

__global__ __launch_bounds__(64) void pnp_hypotheses_kernel(const float *obj, const float *img, const int32_t *count_dev, int n_max, Cam cam,
                                                            int iters, float thr2, unsigned seed, float *poses,
                                                            unsigned long long *best_key) {
    const int n = count_dev ? min(*count_dev, n_max) : n_max;
    if (n < 4) return;
    hypotheses_wave(OneCameraView<CorrGlobal>{CorrGlobal{obj, img, img + 1, 2}, n, cam}, iters, thr2, seed, blockIdx.x * HPW, poses, best_key);
}

// ---- the batched form: frame on blockIdx.y, operands addressed through strides, intrinsics and counts read on the device
struct BatchOperands {
    const float *obj;          // frame f: obj + f * obj_stride, (n_max, 3)
    const float *img;          // frame f: img + f * img_stride; (n_max, 2), or (2, n_max) if coord_major
    const int32_t *count;      // frame f: count[f * count_stride] valid rows (NULL: n_max)
    const float *K;            // (frames, 3, 3) row-major
    int obj_stride, img_stride, count_stride, coord_major, n_max;
    __device__ __forceinline__ int rows(int f) const { return count ? min(count[(size_t)f * count_stride], n_max) : n_max; }
    __device__ __forceinline__ Cam cam(int f) const { return Cam{K[9 * f], K[9 * f + 4], K[9 * f + 2], K[9 * f + 5]}; }
    __device__ __forceinline__ CorrGlobal corr(int f) const {
        const float *uv = img + (size_t)f * img_stride;
        return CorrGlobal{obj + (size_t)f * obj_stride, uv, coord_major ? uv + n_max : uv + 1, coord_major ? 1 : 2};
    }
};

constexpr int BATCH_WAVES = 4;   // waves per workgroup of the batched hypotheses kernel: 64 hypotheses share one staged copy of the frame

// the workgroup's copy of n correspondences in LDS, in CorrLds' layout
__device__ __forceinline__ void stage_rows(const CorrGlobal &g, int n, int ld, float *s_corr) {
    for (int i = threadIdx.x; i < n; i += 64 * BATCH_WAVES) {
        float X[3], uv[2];
        g.load(i, X, uv);
        s_corr[i] = X[0]; s_corr[ld + i] = X[1]; s_corr[2 * ld + i] = X[2];
        s_corr[3 * ld + i] = uv[0]; s_corr[4 * ld + i] = uv[1];
    }
}

// LDS = true: the workgroup stages its frame's correspondences once in LDS (5 n_max floats, dynamic) and every hypothesis scores from
// there; false (frames too large for 64 KiB): from global memory, as the per-frame kernel does.  Same values either way.
template <bool LDS>
__global__ __launch_bounds__(64 * BATCH_WAVES) void pnp_hypotheses_batch_kernel(BatchOperands op, int iters, float thr2, unsigned seed,
                                                                                float *poses, unsigned long long *best_keys) {
    extern __shared__ float s_corr[];
    const int f = blockIdx.y;
    const int n = op.rows(f);
    const Cam cam = op.cam(f);
    if (n < 4 || !(cam.fx > 0.f) || !(cam.fy > 0.f)) return;   // frame-uniform: the key stays 0 and the refit reports failure
    const CorrGlobal g = op.corr(f);
    const int hyp0 = (blockIdx.x * BATCH_WAVES + (threadIdx.x >> 6)) * HPW;
    float *slab = poses + (size_t)f * iters * 12;
    if (LDS) {
        stage_rows(g, n, op.n_max, s_corr);
        __syncthreads();
        hypotheses_wave(OneCameraView<CorrLds>{CorrLds{s_corr, op.n_max}, n, cam}, iters, thr2, seed + (unsigned)f, hyp0, slab, best_keys + f);
    } else {
        hypotheses_wave(OneCameraView<CorrGlobal>{g, n, cam}, iters, thr2, seed + (unsigned)f, hyp0, slab, best_keys + f);
    }
}

// ---- the rig form: rig s on blockIdx.y, its C images are frames s C .. s C + C - 1 of the batched operands; ONE pose per rig.
struct RigOperands {
    BatchOperands op;
    const float *ext;          // rig s, camera c: ext + s * ext_stride + 12 c
    int ext_stride, cameras;   // ext_stride 0: one set of C shared by all rigs
    __device__ __forceinline__ const float *E(int s, int c) const { return ext + (size_t)s * ext_stride + 12 * c; }
    __device__ __forceinline__ bool usable(int f) const { const Cam k = op.cam(f); return k.fx > 0.f && k.fy > 0.f; }
    // rows of the eligible cameras (usable, at least 4 rows) of rig s, in camera order
    __device__ __forceinline__ int total(int s) const {
        int t = 0;
        for (int c = 0; c < cameras; ++c) {
            const int f = s * cameras + c, n = op.rows(f);
            t += (n >= 4 && usable(f)) ? n : 0;
        }
        return t;
    }
};

// STAGED: camera by camera, the workgroup stages the camera's valid rows in LDS (the footprint of the batched kernel whatever C is), its
// 64 hypotheses score them, barrier, next camera.  The four sampled rows are read from global memory either way.
template <bool STAGED>
struct RigView {
    RigOperands rig;
    int s, total;
    float *s_corr;
    struct Scored {
        typename std::conditional<STAGED, CorrLds, CorrGlobal>::type corr;
        int n;
        Cam cam;
        bool scored;
        const float *e;
        __device__ __forceinline__ void carry(const float T[12], float p[12]) const {
            double Td[12], P[12];
            for (int k = 0; k < 12; ++k) Td[k] = (double)T[k];
            ext_compose(e, Td, P);
            for (int k = 0; k < 12; ++k) p[k] = (float)P[k];
        }
    };
    __device__ __forceinline__ int cameras() const { return rig.cameras; }
    __device__ __forceinline__ bool solve(unsigned seed, int hyp, double pose[12]) const {
        int g = (int)(hash_u32(seed, (unsigned)hyp, 4u) % (unsigned)total);   // the camera: proportional to its rows
        int c = 0, n = 0;
        for (; c < rig.cameras; ++c) {
            const int f = s * rig.cameras + c;
            n = rig.op.rows(f);
            if (n < 4 || !rig.usable(f)) continue;
            if (g < n) break;
            g -= n;
        }
        const int f = s * rig.cameras + c;
        double pc[12];
        if (!solve_minimal(rig.op.corr(f), n, rig.op.cam(f), seed, hyp, pc)) return false;
        ext_compose_inverse(rig.E(s, c), pc, pose);
        return true;
    }
    __device__ __forceinline__ Scored score_camera(int c) const {
        const int f = s * rig.cameras + c, n = rig.op.rows(f);
        const bool scored = n >= 1 && rig.usable(f);
        const CorrGlobal g = rig.op.corr(f);
        if constexpr (STAGED) {
            if (scored) {           // rig-uniform, so every wave of the workgroup arrives
                __syncthreads();    // the previous camera's rows have been scored
                stage_rows(g, n, rig.op.n_max, s_corr);
                __syncthreads();
            }
            return Scored{CorrLds{s_corr, rig.op.n_max}, n, rig.op.cam(f), scored, rig.E(s, c)};
        } else {
            return Scored{g, n, rig.op.cam(f), scored, rig.E(s, c)};
        }
    }
};

template <bool STAGED>
__global__ __launch_bounds__(64 * BATCH_WAVES) void pnp_hypotheses_rig_kernel(RigOperands rig, int iters, float thr2, unsigned seed,
                                                                              float *poses, unsigned long long *best_keys) {
    extern __shared__ float s_corr[];
    const int s = blockIdx.y;
    const int total = rig.total(s);
    if (total == 0) return;   // rig-uniform: no eligible camera, the key stays 0 and the refit reports failure
    const int hyp0 = (blockIdx.x * BATCH_WAVES + (threadIdx.x >> 6)) * HPW;
    hypotheses_wave(RigView<STAGED>{rig, s, total, s_corr}, iters, thr2, seed + (unsigned)s, hyp0, poses + (size_t)s * iters * 12, best_keys + s);
}

// ---- refit: Levenberg-Marquardt on the inliers of the winning hypothesis
constexpr int NACC = 28;  // 21 (upper JtJ) + 6 (Jt r) + 1 (cost)

// the normal equations gain one residual pair: rows J0, J1 of its 2x6 Jacobian, residuals r0, r1
__device__ __forceinline__ void accumulate_rows(const double J0[6], const double J1[6], double r0, double r1, double acc[NACC]) {
    int k = 0;
    for (int i = 0; i < 6; ++i)
        for (int j = i; j < 6; ++j) acc[k++] += J0[i] * J0[j] + J1[i] * J1[j];
    for (int i = 0; i < 6; ++i) acc[21 + i] += J0[i] * r0 + J1[i] * r1;
    acc[27] += r0 * r0 + r1 * r1;
}

__device__ void accumulate(const double R[9], const double t[3], const float *X, const float *uv, const Cam &cam, double acc[NACC]) {
    const double x = R[0] * X[0] + R[1] * X[1] + R[2] * X[2] + t[0], y = R[3] * X[0] + R[4] * X[1] + R[5] * X[2] + t[1],
                 z = R[6] * X[0] + R[7] * X[1] + R[8] * X[2] + t[2];
    const double iz = 1.0 / z;
    const double r0 = cam.fx * x * iz + cam.cx - uv[0], r1 = cam.fy * y * iz + cam.cy - uv[1];
    // d(pi)/dY (2x3) times [-[Y]x | I] (3x6)
    const double a00 = cam.fx * iz, a02 = -cam.fx * x * iz * iz, a11 = cam.fy * iz, a12 = -cam.fy * y * iz * iz;
    // -[Y]x = [[0, z, -y], [-z, 0, x], [y, -x, 0]]
    const double J0[6] = {a02 * y, a00 * z - a02 * x, -a00 * y, a00, 0.0, a02};
    const double J1[6] = {-a11 * z + a12 * y, -a12 * x, a11 * x, 0.0, a11, a12};
    accumulate_rows(J0, J1, r0, r1, acc);
}

// a row of camera c of a rig: the pose (R, t) is the RIG's; the point is carried on into the camera, Y_c = R_c (R X + t) + t_c, and the
// Jacobian with respect to the rig's left-multiplied increment is d(pi)/dY_c . R_c . [-[Y_rig]x | I]
__device__ void accumulate_rig(const double R[9], const double t[3], const float *e, const float *X, const float *uv, const Cam &cam,
                               double acc[NACC]) {
    const double xr = R[0] * X[0] + R[1] * X[1] + R[2] * X[2] + t[0], yr = R[3] * X[0] + R[4] * X[1] + R[5] * X[2] + t[1],
                 zr = R[6] * X[0] + R[7] * X[1] + R[8] * X[2] + t[2];
    const double x = (double)e[0] * xr + (double)e[1] * yr + (double)e[2] * zr + (double)e[9],
                 y = (double)e[3] * xr + (double)e[4] * yr + (double)e[5] * zr + (double)e[10],
                 z = (double)e[6] * xr + (double)e[7] * yr + (double)e[8] * zr + (double)e[11];
    const double iz = 1.0 / z;
    const double r0 = cam.fx * x * iz + cam.cx - uv[0], r1 = cam.fy * y * iz + cam.cy - uv[1];
    const double a00 = cam.fx * iz, a02 = -cam.fx * x * iz * iz, a11 = cam.fy * iz, a12 = -cam.fy * y * iz * iz;
    double A0[3], A1[3];   // d(pi)/dY_c . R_c
    for (int j = 0; j < 3; ++j) {
        A0[j] = a00 * (double)e[j] + a02 * (double)e[6 + j];
        A1[j] = a11 * (double)e[3 + j] + a12 * (double)e[6 + j];
    }
    const double J0[6] = {A0[2] * yr - A0[1] * zr, A0[0] * zr - A0[2] * xr, A0[1] * xr - A0[0] * yr, A0[0], A0[1], A0[2]};
    const double J1[6] = {A1[2] * yr - A1[1] * zr, A1[0] * zr - A1[2] * xr, A1[1] * xr - A1[0] * yr, A1[0], A1[1], A1[2]};
    accumulate_rows(J0, J1, r0, r1, acc);
}

// What the refit body works on: the cameras of the body whose pose is refitted (one for a frame of its own, C for a rig), and where
// the outcome goes.
template <class Corr>
struct OneFrameView {
    Corr corr_;
    int n, n_max;
    Cam cam_;
    float *pose_out;
    int32_t *result;   // [0] success, [1] inliers, [2] hypothesis
    uint8_t *mask_;
    struct Camera {
        Corr corr;
        int n, n_max;
        Cam cam;
        uint8_t *mask;
        bool scored;
        __device__ __forceinline__ void carry(const double T[12], float p[12]) const {
            for (int k = 0; k < 12; ++k) p[k] = (float)T[k];
        }
        __device__ __forceinline__ void accumulate_row(const double R[9], const double t[3], const float *X, const float *uv, double acc[NACC]) const {
            accumulate(R, t, X, uv, cam, acc);
        }
        __device__ __forceinline__ void set_inliers(int) const {}
    };
    __device__ __forceinline__ int cameras() const { return 1; }
    __device__ __forceinline__ bool solvable() const { return n >= 4; }
    __device__ __forceinline__ Camera camera(int) const { return Camera{corr_, n, n_max, cam_, mask_, true}; }
    __device__ __forceinline__ void fail() const {   // one thread
        result[0] = 0; result[1] = 0; result[2] = -1;
        for (int k = 0; k < 12; ++k) pose_out[k] = (k == 0 || k == 4 || k == 8) ? 1.f : 0.f;
    }
    __device__ __forceinline__ void succeed(const double pose[12], int inliers, int hyp) const {   // one thread
        for (int k = 0; k < 12; ++k) pose_out[k] = (float)pose[k];
        result[0] = 1; result[1] = inliers; result[2] = hyp;
    }
};

struct RigRefitView {
    RigOperands rig;
    int s;
    float *rig_pose, *pose;          // of this rig (12), of image 0 of this rig (C x 12)
    int32_t *rig_result, *result;    // of this rig (3), of image 0 of this rig (C x 3)
    uint8_t *mask_;                  // of image 0 of this rig (C x n_max)
    struct Camera {
        CorrGlobal corr;
        int n, n_max;
        Cam cam;
        uint8_t *mask;
        bool scored;
        const float *e;
        int32_t *result;
        __device__ __forceinline__ void carry(const double T[12], float p[12]) const {
            double P[12];
            ext_compose(e, T, P);
            for (int k = 0; k < 12; ++k) p[k] = (float)P[k];
        }
        __device__ __forceinline__ void accumulate_row(const double R[9], const double t[3], const float *X, const float *uv, double acc[NACC]) const {
            accumulate_rig(R, t, e, X, uv, cam, acc);
        }
        __device__ __forceinline__ void set_inliers(int c) const { result[1] = c; }
    };
    __device__ __forceinline__ int cameras() const { return rig.cameras; }
    __device__ __forceinline__ bool solvable() const { return true; }   // a rig without an eligible camera has key 0
    __device__ __forceinline__ Camera camera(int c) const {
        const int f = s * rig.cameras + c, n = rig.op.rows(f);
        return Camera{rig.op.corr(f), n, rig.op.n_max, rig.op.cam(f), mask_ + (size_t)c * rig.op.n_max, n >= 1 && rig.usable(f), rig.E(s, c),
                      result + 3 * c};
    }
    __device__ __forceinline__ void fail() const {
        for (int c = -1; c < rig.cameras; ++c) {
            int32_t *r = c < 0 ? rig_result : result + 3 * c;
            float *p = c < 0 ? rig_pose : pose + 12 * c;
            r[0] = 0; r[1] = 0; r[2] = -1;
            for (int k = 0; k < 12; ++k) p[k] = (k == 0 || k == 4 || k == 8) ? 1.f : 0.f;
        }
    }
    // the rig's pose rounded once; every image's pose is the composition E_c o (that float32 pose), rounded once: an unscored camera
    // (no rows, unusable intrinsics) still gets its pose, with the 0 inliers the body left in its result
    __device__ __forceinline__ void succeed(const double T[12], int inliers, int hyp) const {
        double Tf[12];
        for (int k = 0; k < 12; ++k) {
            rig_pose[k] = (float)T[k];
            Tf[k] = (double)rig_pose[k];
        }
        rig_result[0] = 1; rig_result[1] = inliers; rig_result[2] = hyp;
        for (int c = 0; c < rig.cameras; ++c) {
            double P[12];
            ext_compose(rig.E(s, c), Tf, P);
            for (int k = 0; k < 12; ++k) pose[12 * c + k] = (float)P[k];
            result[3 * c] = 1; result[3 * c + 2] = hyp;
        }
    }
};

// One workgroup of 256 threads refits one body (a frame, a rig) on the inliers of all its cameras.  The body of all refit kernels.
template <class View>
__device__ __forceinline__ void refine_workgroup(const View &view, float thr2, const float *poses, const unsigned long long *best_key,
                                                 int lm_iters) {
    __shared__ double s_red[4][NACC];
    __shared__ double s_sys[NACC];     // reduced normal equations of the candidate pose
    __shared__ double s_pose[12], s_cand[12];
    __shared__ int s_cnt[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const unsigned long long key = *best_key;
    const int cnt_best = (int)(key >> 32);
    const int hyp = (int)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull));
    for (int c = 0; c < view.cameras(); ++c) {
        const auto cv = view.camera(c);
        for (int i = tid; i < cv.n_max; i += 256) cv.mask[i] = 0;
    }
    if (!view.solvable() || key == 0ull || cnt_best < 4) {
        if (tid == 0) view.fail();
        return;
    }
    double pd[12];
    for (int k = 0; k < 12; ++k) pd[k] = (double)poses[(size_t)hyp * 12 + k];
    if (tid < 12) s_pose[tid] = pd[tid];
    // inlier masks of the RANSAC model (what cv2 returns as `inliers`), camera by camera
    int n_in = 0;
    for (int cc = 0; cc < view.cameras(); ++cc) {
        const auto cv = view.camera(cc);
        int c = 0;
        if (cv.scored) {
            float pf[12];
            cv.carry(pd, pf);
            for (int i = tid; i < cv.n; i += 256) {
                float Xi[3], uvi[2];
                cv.corr.load(i, Xi, uvi);
                const bool in = inlier(pf, Xi, uvi, cv.cam, thr2);
                cv.mask[i] = in ? 1 : 0;
                c += in ? 1 : 0;
            }
        }
        for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
        if (lane == 0) s_cnt[wv] = c;
        __syncthreads();
        const int n_cam = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
        if (tid == 0) cv.set_inliers(n_cam);
        n_in += n_cam;
        if (cc + 1 < view.cameras()) __syncthreads();   // s_cnt is reused
    }

    // normal equations at `pose` over the inliers, reduced in a fixed order: camera-major, thread-strided partials -> wave butterflies -> 4 waves
    auto reduce_at = [&](const double *pose) {
        double acc[NACC];
        for (int k = 0; k < NACC; ++k) acc[k] = 0.0;
        double R[9], t[3];
        for (int k = 0; k < 9; ++k) R[k] = pose[k];
        for (int k = 0; k < 3; ++k) t[k] = pose[9 + k];
        for (int cc = 0; cc < view.cameras(); ++cc) {
            const auto cv = view.camera(cc);
            if (!cv.scored) continue;
            for (int i = tid; i < cv.n; i += 256)
                if (cv.mask[i]) {
                    float Xi[3], uvi[2];
                    cv.corr.load(i, Xi, uvi);
                    cv.accumulate_row(R, t, Xi, uvi, acc);
                }
        }
        for (int k = 0; k < NACC; ++k) {
            const double v = wave_sum_d(acc[k]);
            if (lane == 0) s_red[wv][k] = v;
        }
        __syncthreads();
        if (tid < NACC) s_sys[tid] = (s_red[0][tid] + s_red[1][tid]) + (s_red[2][tid] + s_red[3][tid]);
        __syncthreads();
    };

    __syncthreads();
    reduce_at(s_pose);
    double H[21], g[6], cost = 0.0, lam = 1e-3;   // thread 0's copy of the accepted system
    if (tid == 0) {
        for (int k = 0; k < 21; ++k) H[k] = s_sys[k];
        for (int k = 0; k < 6; ++k) g[k] = s_sys[21 + k];
        cost = s_sys[27];
    }
    for (int it = 0; it < lm_iters; ++it) {
        if (tid == 0) {
            // (H + lam diag(H) + eps I) d = -g by Gaussian elimination with partial pivoting
            double A[6][7];
            int k = 0;
            for (int i = 0; i < 6; ++i)
                for (int j = i; j < 6; ++j) { A[i][j] = H[k]; A[j][i] = H[k]; ++k; }
            for (int i = 0; i < 6; ++i) { A[i][i] += lam * A[i][i] + 1e-12; A[i][6] = -g[i]; }
            bool okk = true;
            for (int col = 0; col < 6; ++col) {
                int piv = col;
                for (int r = col + 1; r < 6; ++r)
                    if (fabs(A[r][col]) > fabs(A[piv][col])) piv = r;
                if (fabs(A[piv][col]) < 1e-300) { okk = false; break; }
                if (piv != col)
                    for (int j = 0; j < 7; ++j) { const double tmp = A[col][j]; A[col][j] = A[piv][j]; A[piv][j] = tmp; }
                for (int r = col + 1; r < 6; ++r) {
                    const double fct = A[r][col] / A[col][col];
                    for (int j = col; j < 7; ++j) A[r][j] -= fct * A[col][j];
                }
            }
            double d[6] = {0, 0, 0, 0, 0, 0};
            if (okk)
                for (int i = 5; i >= 0; --i) {
                    double sacc = A[i][6];
                    for (int j = i + 1; j < 6; ++j) sacc -= A[i][j] * d[j];
                    d[i] = sacc / A[i][i];
                }
            // candidate = exp(omega) * pose, t' = exp(omega) t + delta (Rodrigues)
            const double wx = d[0], wy = d[1], wz = d[2];
            const double th = sqrt(wx * wx + wy * wy + wz * wz);
            double E[9];
            const double W[9] = {0, -wz, wy, wz, 0, -wx, -wy, wx, 0};
            double W2[9];
            for (int r = 0; r < 3; ++r)
                for (int cc = 0; cc < 3; ++cc) W2[3 * r + cc] = W[3 * r] * W[cc] + W[3 * r + 1] * W[3 + cc] + W[3 * r + 2] * W[6 + cc];
            const double ka = th < 1e-12 ? 1.0 : sin(th) / th, kb = th < 1e-12 ? 0.0 : (1.0 - cos(th)) / (th * th);
            for (int k2 = 0; k2 < 9; ++k2) E[k2] = ((k2 % 4) == 0 ? 1.0 : 0.0) + ka * W[k2] + kb * W2[k2];
            for (int r = 0; r < 3; ++r) {
                for (int cc = 0; cc < 3; ++cc)
                    s_cand[3 * r + cc] = E[3 * r] * s_pose[cc] + E[3 * r + 1] * s_pose[3 + cc] + E[3 * r + 2] * s_pose[6 + cc];
                s_cand[9 + r] = E[3 * r] * s_pose[9] + E[3 * r + 1] * s_pose[10] + E[3 * r + 2] * s_pose[11] + d[3 + r];
            }
        }
        __syncthreads();
        reduce_at(s_cand);
        if (tid == 0) {
            const double cn = s_sys[27];
            if (cn == cn && cn < cost) {   // accept
                for (int k = 0; k < 12; ++k) s_pose[k] = s_cand[k];
                for (int k = 0; k < 21; ++k) H[k] = s_sys[k];
                for (int k = 0; k < 6; ++k) g[k] = s_sys[21 + k];
                cost = cn;
                lam = fmax(lam * 0.1, 1e-9);
            } else {
                lam = fmin(lam * 10.0, 1e6);
            }
        }
        __syncthreads();
    }
    if (tid == 0) view.succeed(s_pose, n_in, hyp);
}

__global__ __launch_bounds__(256) void pnp_refine_kernel(const float *obj, const float *img, const int32_t *count_dev, int n_max, Cam cam,
                                                         float thr2, const float *poses, const unsigned long long *best_key, int lm_iters,
                                                         float *pose_out, int32_t *result, uint8_t *mask) {
    const int n = count_dev ? min(*count_dev, n_max) : n_max;
    refine_workgroup(OneFrameView<CorrGlobal>{CorrGlobal{obj, img, img + 1, 2}, n, n_max, cam, pose_out, result, mask}, thr2, poses, best_key,
                     lm_iters);
}

// frame f = blockIdx.x: pose_out (frames, 12), result (frames, 3), mask (frames, n_max).  A frame the hypotheses kernel left at once
// (count < 4, unusable intrinsics) has key 0 and takes the failure exit.
__global__ __launch_bounds__(256) void pnp_refine_batch_kernel(BatchOperands op, int iters, float thr2, const float *poses,
                                                               const unsigned long long *best_keys, int lm_iters, float *pose_out,
                                                               int32_t *result, uint8_t *mask) {
    const int f = blockIdx.x;
    refine_workgroup(OneFrameView<CorrGlobal>{op.corr(f), op.rows(f), op.n_max, op.cam(f), pose_out + 12 * f, result + 3 * f,
                                              mask + (size_t)f * op.n_max},
                     thr2, poses + (size_t)f * iters * 12, best_keys + f, lm_iters);
}

// rig s = blockIdx.x: rig_pose (rigs, 12), rig_result (rigs, 3); per image pose (rigs C, 12), result (rigs C, 3), mask (rigs C, n_max)
__global__ __launch_bounds__(256) void pnp_refine_rig_kernel(RigOperands rig, int iters, float thr2, const float *poses,
                                                             const unsigned long long *best_keys, int lm_iters, float *rig_pose,
                                                             int32_t *rig_result, float *pose, int32_t *result, uint8_t *mask) {
    const int s = blockIdx.x;
    const size_t f0 = (size_t)s * rig.cameras;
    refine_workgroup(RigRefitView{rig, s, rig_pose + 12 * s, pose + 12 * f0, rig_result + 3 * s, result + 3 * f0, mask + f0 * rig.op.n_max}, thr2,
                     poses + (size_t)s * iters * 12, best_keys + s, lm_iters);
}

// ---- pose covariance: the Gauss-Newton covariance of the refit's least-squares problem at the pose that was RETURNED (float32), over the
// consensus set the solver wrote into the masks.  H = sum J^T J and cost = sum |r|^2 through accumulate / accumulate_rig, sigma^2 =
// cost / (2 n - 6) (or the caller's), info = H / sigma^2, cov = sigma^2 H^-1 by a Cholesky factorisation of the unit-diagonal
// D^-1/2 H D^-1/2.  One wave per body, no LDS, no barrier: camera-major, lane-strided partials, wave_sum_d; lane 0 factorises and stores.
constexpr int COV_WAVES = 4;   // bodies per workgroup of the batched and the rig kernel

// What the covariance body works on: the scored cameras of the body (usable intrinsics), their rows, masks and row Jacobians.
struct FrameCovView {
    CorrGlobal corr_;
    int n;
    Cam cam_;
    const uint8_t *mask_;
    struct Camera {
        CorrGlobal corr;
        int n;
        Cam cam;
        const uint8_t *mask;
        bool scored;
        __device__ __forceinline__ double depth(const double R[9], const double t[3], const float *X) const {
            return R[6] * X[0] + R[7] * X[1] + R[8] * X[2] + t[2];
        }
        __device__ __forceinline__ void accumulate_row(const double R[9], const double t[3], const float *X, const float *uv, double acc[NACC]) const {
            accumulate(R, t, X, uv, cam, acc);
        }
    };
    __device__ __forceinline__ int cameras() const { return 1; }
    __device__ __forceinline__ Camera camera(int) const { return Camera{corr_, n, cam_, mask_, cam_.fx > 0.f && cam_.fy > 0.f}; }
};

struct RigCovView {
    RigOperands rig;
    int s;
    const uint8_t *mask_;   // of image 0 of this rig (C x n_max)
    struct Camera {
        CorrGlobal corr;
        int n;
        Cam cam;
        const uint8_t *mask;
        bool scored;
        const float *e;
        __device__ __forceinline__ double depth(const double R[9], const double t[3], const float *X) const {   // as accumulate_rig carries the point
            const double xr = R[0] * X[0] + R[1] * X[1] + R[2] * X[2] + t[0], yr = R[3] * X[0] + R[4] * X[1] + R[5] * X[2] + t[1],
                         zr = R[6] * X[0] + R[7] * X[1] + R[8] * X[2] + t[2];
            return (double)e[6] * xr + (double)e[7] * yr + (double)e[8] * zr + (double)e[11];
        }
        __device__ __forceinline__ void accumulate_row(const double R[9], const double t[3], const float *X, const float *uv, double acc[NACC]) const {
            accumulate_rig(R, t, e, X, uv, cam, acc);
        }
    };
    __device__ __forceinline__ int cameras() const { return rig.cameras; }
    __device__ __forceinline__ Camera camera(int c) const {
        const int f = s * rig.cameras + c;
        return Camera{rig.op.corr(f), rig.op.rows(f), rig.op.cam(f), mask_ + (size_t)c * rig.op.n_max, rig.usable(f), rig.E(s, c)};
    }
};

__device__ __forceinline__ bool finite_d(double v) { return fabs(v) <= 1.7976931348623157e308; }   // false for NaN and Inf

// One wave, one body.  pose (12) and result (3) are the solver's outputs for the body; sigma_px <= 0: estimate the pixel variance.
// cov, info (36 each, row-major, exactly symmetric), stat (4) = [ok, n, sigma_hat^2, min_pivot].  ok = 0 writes zeros, never NaN or Inf.
template <class View>
__device__ __forceinline__ void covariance_body(const View &view, const float *pose, const int32_t *result, float sigma_px, double *cov,
                                                double *info, double *stat) {
    const int lane = threadIdx.x & 63;
    double acc[NACC];
    for (int k = 0; k < NACC; ++k) acc[k] = 0.0;
    double R[9], t[3];
    for (int k = 0; k < 9; ++k) R[k] = (double)pose[k];
    for (int k = 0; k < 3; ++k) t[k] = (double)pose[9 + k];
    const bool solved = result[0] != 0;   // body-uniform
    bool any_camera = false;
    int used = 0;
    if (solved)
        for (int cc = 0; cc < view.cameras(); ++cc) {
            const auto cv = view.camera(cc);
            if (!cv.scored) continue;
            any_camera = true;
            for (int i = lane; i < cv.n; i += 64)
                if (cv.mask[i]) {
                    float Xi[3], uvi[2];
                    cv.corr.load(i, Xi, uvi);
                    if (cv.depth(R, t, Xi) > 1e-6) {   // the solver's inlier rule: a NaN depth compares false
                        cv.accumulate_row(R, t, Xi, uvi, acc);
                        ++used;
                    }
                }
        }
    for (int k = 0; k < NACC; ++k) acc[k] = wave_sum_d(acc[k]);
    for (int o = 32; o > 0; o >>= 1) used += __shfl_xor(used, o, 64);
    if (lane != 0) return;

    double H[6][6], C[6][6], I[6][6];
    {
        int k = 0;
        for (int i = 0; i < 6; ++i)
            for (int j = i; j < 6; ++j) { H[i][j] = acc[k]; H[j][i] = acc[k]; ++k; }
    }
    const double cost = acc[27];
    const int dof = 2 * used - 6;
    bool ok = solved && any_camera;
    for (int k = 0; k < NACC; ++k) ok = ok && finite_d(acc[k]);
    const double sigma_hat2 = (ok && dof > 0) ? cost / (double)dof : 0.0;
    const double sigma2 = sigma_px > 0.f ? (double)sigma_px * (double)sigma_px : sigma_hat2;
    ok = ok && (sigma_px > 0.f || dof > 0) && sigma2 > 0.0;
    double d[6];
    for (int i = 0; i < 6; ++i) {
        ok = ok && H[i][i] > 0.0;
        d[i] = ok ? 1.0 / sqrt(H[i][i]) : 0.0;
    }
    // Cholesky of Hs = D^-1/2 H D^-1/2 (unit diagonal), then L^-1: fixed trip counts, a failed pivot only clears `ok`
    double L[6][6], Li[6][6], min_pivot = 1.0;
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) { L[i][j] = 0.0; Li[i][j] = 0.0; }
    for (int j = 0; j < 6; ++j) {
        double sacc = 1.0;
        for (int k = 0; k < j; ++k) sacc -= L[j][k] * L[j][k];
        const bool good = sacc > 1e-12;   // false for NaN
        ok = ok && good;
        min_pivot = (good && sacc < min_pivot) ? sacc : min_pivot;
        const double piv = good ? sqrt(sacc) : 1.0;
        L[j][j] = piv;
        for (int i = j + 1; i < 6; ++i) {
            double v = H[i][j] * d[i] * d[j];
            for (int k = 0; k < j; ++k) v -= L[i][k] * L[j][k];
            L[i][j] = v / piv;
        }
    }
    for (int j = 0; j < 6; ++j) {   // column j of L^-1 by forward substitution
        Li[j][j] = 1.0 / L[j][j];
        for (int i = j + 1; i < 6; ++i) {
            double v = 0.0;
            for (int k = j; k < i; ++k) v -= L[i][k] * Li[k][j];
            Li[i][j] = v / L[i][i];
        }
    }
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j <= i; ++j) {   // one triangle, mirrored: Hs^-1 = L^-T L^-1
            double v = 0.0;
            for (int k = i; k < 6; ++k) v += Li[k][i] * Li[k][j];
            const double c = sigma2 * (d[i] * d[j] * v), f = ok ? H[i][j] / sigma2 : 0.0;
            ok = ok && finite_d(c) && finite_d(f);
            C[i][j] = c; C[j][i] = c;
            I[i][j] = f; I[j][i] = f;
        }
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) {
            cov[6 * i + j] = ok ? C[i][j] : 0.0;
            info[6 * i + j] = ok ? I[i][j] : 0.0;
        }
    stat[0] = ok ? 1.0 : 0.0;
    stat[1] = (double)used;
    stat[2] = finite_d(sigma_hat2) ? sigma_hat2 : 0.0;
    stat[3] = ok ? min_pivot : 0.0;
}

__global__ __launch_bounds__(64) void pose_covariance_kernel(const float *obj, const float *img, const int32_t *count_dev, int n_max, Cam cam,
                                                             const float *pose, const int32_t *result, const uint8_t *mask, float sigma_px,
                                                             double *cov, double *info, double *stat) {
    const int n = count_dev ? min(*count_dev, n_max) : n_max;
    covariance_body(FrameCovView{CorrGlobal{obj, img, img + 1, 2}, n, cam, mask}, pose, result, sigma_px, cov, info, stat);
}

// frame f = one wave: pose (frames, 12), result (frames, 3), mask (frames, n_max) -> cov, info (frames, 36), stat (frames, 4)
__global__ __launch_bounds__(64 * COV_WAVES) void pose_covariance_batch_kernel(BatchOperands op, int frames, const float *pose,
                                                                               const int32_t *result, const uint8_t *mask, float sigma_px,
                                                                               double *cov, double *info, double *stat) {
    const int f = blockIdx.x * COV_WAVES + (threadIdx.x >> 6);
    if (f >= frames) return;   // wave-uniform; the body has no barrier
    covariance_body(FrameCovView{op.corr(f), op.rows(f), op.cam(f), mask + (size_t)f * op.n_max}, pose + 12 * f, result + 3 * f, sigma_px,
                    cov + 36 * (size_t)f, info + 36 * (size_t)f, stat + 4 * (size_t)f);
}

// rig s = one wave: rig_pose (rigs, 12), rig_result (rigs, 3), mask (rigs C, n_max) -> cov, info (rigs, 36), stat (rigs, 4)
__global__ __launch_bounds__(64 * COV_WAVES) void pose_covariance_rig_kernel(RigOperands rig, int rigs, const float *rig_pose,
                                                                             const int32_t *rig_result, const uint8_t *mask, float sigma_px,
                                                                             double *cov, double *info, double *stat) {
    const int s = blockIdx.x * COV_WAVES + (threadIdx.x >> 6);
    if (s >= rigs) return;
    covariance_body(RigCovView{rig, s, mask + (size_t)s * rig.cameras * rig.op.n_max}, rig_pose + 12 * s, rig_result + 3 * s, sigma_px,
                    cov + 36 * (size_t)s, info + 36 * (size_t)s, stat + 4 * (size_t)s);
}

// ---- registration errors of B poses (evaluation/eval_all.py:16-22): P_diff = inv(P_pred) P_gt, RTE = |t|, RRE = sum |euler 'xzy'| in degrees
// (pose_errors.h: the body, shared with cofi_eval_monitors)
template <class T>
__global__ __launch_bounds__(64) void pose_errors_kernel(const float *pose, const T *P_gt, int frames, double *out) {
    const int f = blockIdx.x * 64 + threadIdx.x;
    if (f >= frames) return;
    pose_errors_frame(pose + 12 * f, P_gt + 16 * f, out + 2 * f, out + 2 * f + 1);
}

// ---- normalised estimation error squared of B poses against ground truth, in the tangent space of the covariance: omega =
// log(R_gt R_est^T), v = t_gt - exp(omega) t_est, e = (omega, v), nees = e^T info e; NaN where stat[0] == 0.  One thread per body, fp64.
template <class T>
__global__ __launch_bounds__(64) void pose_nees_kernel(const float *pose, const T *P_gt, const double *info, const double *stat, int frames,
                                                       double *out) {
    const int f = blockIdx.x * 64 + threadIdx.x;
    if (f >= frames) return;
    if (stat[4 * (size_t)f] == 0.0) {
        out[f] = __builtin_nan("");
        return;
    }
    const float *p = pose + 12 * f;
    const T *G = P_gt + 16 * f;
    double M[9];   // R_gt R_est^T
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c)
            M[3 * r + c] = (double)G[4 * r] * (double)p[3 * c] + (double)G[4 * r + 1] * (double)p[3 * c + 1] + (double)G[4 * r + 2] * (double)p[3 * c + 2];
    const double a[3] = {0.5 * (M[7] - M[5]), 0.5 * (M[2] - M[6]), 0.5 * (M[3] - M[1])};   // sin(theta) times the axis
    const double sn = sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]), cs = 0.5 * (M[0] + M[4] + M[8] - 1.0);
    const double th = atan2(sn, cs), scale = sn > 1e-12 ? th / sn : 1.0;
    double e[6];
    for (int k = 0; k < 3; ++k) e[k] = a[k] * scale;
    // exp(omega) by Rodrigues, as the refit builds it
    const double wx = e[0], wy = e[1], wz = e[2];
    const double W[9] = {0, -wz, wy, wz, 0, -wx, -wy, wx, 0};
    double W2[9];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) W2[3 * r + c] = W[3 * r] * W[c] + W[3 * r + 1] * W[3 + c] + W[3 * r + 2] * W[6 + c];
    const double ka = th < 1e-12 ? 1.0 : sin(th) / th, kb = th < 1e-12 ? 0.0 : (1.0 - cos(th)) / (th * th);
    for (int r = 0; r < 3; ++r) {
        double Er[3];
        for (int c = 0; c < 3; ++c) Er[c] = ((r == c) ? 1.0 : 0.0) + ka * W[3 * r + c] + kb * W2[3 * r + c];
        e[3 + r] = (double)G[4 * r + 3] - (Er[0] * (double)p[9] + Er[1] * (double)p[10] + Er[2] * (double)p[11]);
    }
    const double *A = info + 36 * (size_t)f;
    double q = 0.0;
    for (int i = 0; i < 6; ++i) {
        double row = 0.0;
        for (int j = 0; j < 6; ++j) row += A[6 * i + j] * e[j];
        q += e[i] * row;
    }
    out[f] = q;
}

}  // namespace

extern "C" size_t cofi_pnp_ransac_workspace(int iterations) {
    return iterations > 0 ? 64 + (size_t)iterations * 12 * sizeof(float) : 0;
}

extern "C" int cofi_pnp_ransac(const float *obj, const float *img, const int32_t *count_dev, int n_max, float fx, float fy, float cx,
                               float cy, int iterations, float reproj_err, unsigned seed, int refine_iters, void *ws, size_t ws_bytes,
                               float *pose, int32_t *result, uint8_t *inlier_mask, cofi_stream_t stream) {
    if (!obj || !img || !pose || !result || !inlier_mask || n_max <= 0 || iterations <= 0 || !(reproj_err > 0.f) || !(fx > 0.f) || !(fy > 0.f) ||
        refine_iters < 0)
        return COFI_EINVAL;
    if (!ws || ws_bytes < cofi_pnp_ransac_workspace(iterations) || ((uintptr_t)ws & 15)) return COFI_EWORKSPACE;
    hipStream_t s = cofi_s(stream);
    unsigned long long *key = (unsigned long long *)ws;
    float *poses = (float *)((char *)ws + 64);
    if (hipError_t e = hipMemsetAsync(key, 0, 8, s); e != hipSuccess) return (int)e;
    const Cam cam{fx, fy, cx, cy};
    hipLaunchKernelGGL(pnp_hypotheses_kernel, dim3(cofi_cdiv(iterations, HPW)), dim3(64), 0, s, obj, img, count_dev, n_max, cam, iterations,
                       reproj_err * reproj_err, seed, poses, key);
    hipLaunchKernelGGL(pnp_refine_kernel, dim3(1), dim3(256), 0, s, obj, img, count_dev, n_max, cam, reproj_err * reproj_err, poses, key,
                       refine_iters, pose, result, inlier_mask);
    return cofi_launch_status();
}

// workspace of the batched call: one consensus key per frame (padded to 64 bytes), then one slab of iterations x 12 floats per frame
static size_t batch_key_bytes(int frames) { return ((size_t)frames * 8 + 63) / 64 * 64; }

extern "C" size_t cofi_pnp_ransac_batch_workspace(int iterations, int frames) {
    return iterations > 0 && frames > 0 ? batch_key_bytes(frames) + (size_t)frames * iterations * 12 * sizeof(float) : 0;
}

extern "C" int cofi_pnp_ransac_batch(const float *obj, int obj_frame_stride, const float *img, int img_frame_stride, int coord_major,
                                     const int32_t *count_dev, int count_stride, const float *K_dev, int n_max, int frames, int iterations,
                                     float reproj_err, unsigned seed, int refine_iters, void *ws, size_t ws_bytes, float *pose,
                                     int32_t *result, uint8_t *inlier_mask, cofi_stream_t stream) {
    if (!obj || !img || !K_dev || !pose || !result || !inlier_mask || n_max <= 0 || frames <= 0 || frames > 65535 || iterations <= 0 ||
        !(reproj_err > 0.f) || refine_iters < 0 || obj_frame_stride < 3 * n_max || img_frame_stride < 2 * n_max || (count_dev && count_stride < 1))
        return COFI_EINVAL;
    if (!ws || ws_bytes < cofi_pnp_ransac_batch_workspace(iterations, frames) || ((uintptr_t)ws & 15)) return COFI_EWORKSPACE;
    hipStream_t s = cofi_s(stream);
    unsigned long long *keys = (unsigned long long *)ws;
    float *poses = (float *)((char *)ws + batch_key_bytes(frames));
    if (hipError_t e = hipMemsetAsync(keys, 0, batch_key_bytes(frames), s); e != hipSuccess) return (int)e;
    const BatchOperands op{obj, img, count_dev, K_dev, obj_frame_stride, img_frame_stride, count_stride, coord_major ? 1 : 0, n_max};
    const float thr2 = reproj_err * reproj_err;
    const dim3 grid(cofi_cdiv(iterations, HPW * BATCH_WAVES), frames), block(64 * BATCH_WAVES);
    const size_t lds = (size_t)n_max * 5 * sizeof(float);
    if (lds <= 64 * 1024)
        hipLaunchKernelGGL(pnp_hypotheses_batch_kernel<true>, grid, block, lds, s, op, iterations, thr2, seed, poses, keys);
    else
        hipLaunchKernelGGL(pnp_hypotheses_batch_kernel<false>, grid, block, 0, s, op, iterations, thr2, seed, poses, keys);
    hipLaunchKernelGGL(pnp_refine_batch_kernel, dim3(frames), dim3(256), 0, s, op, iterations, thr2, poses, keys, refine_iters, pose, result,
                       inlier_mask);
    return cofi_launch_status();
}

// workspace of the rig call: the batched layout with one key and one slab per RIG (the slab holds rig poses)
extern "C" size_t cofi_pnp_ransac_rig_workspace(int iterations, int rigs) { return cofi_pnp_ransac_batch_workspace(iterations, rigs); }

extern "C" int cofi_pnp_ransac_rig(const float *obj, int obj_frame_stride, const float *img, int img_frame_stride, int coord_major,
                                   const int32_t *count_dev, int count_stride, const float *K_dev, const float *ext_dev, int ext_rig_stride,
                                   int n_max, int cameras, int rigs, int iterations, float reproj_err, unsigned seed, int refine_iters,
                                   void *ws, size_t ws_bytes, float *rig_pose, int32_t *rig_result, float *pose, int32_t *result,
                                   uint8_t *inlier_mask, cofi_stream_t stream) {
    if (!obj || !img || !K_dev || !ext_dev || !rig_pose || !rig_result || !pose || !result || !inlier_mask || n_max <= 0 || cameras <= 0 ||
        rigs <= 0 || (long long)rigs * cameras > 65535 || iterations <= 0 || !(reproj_err > 0.f) || refine_iters < 0 ||
        obj_frame_stride < 3 * n_max || img_frame_stride < 2 * n_max || (count_dev && count_stride < 1) ||
        (ext_rig_stride != 0 && ext_rig_stride < 12 * cameras))
        return COFI_EINVAL;
    if (!ws || ws_bytes < cofi_pnp_ransac_rig_workspace(iterations, rigs) || ((uintptr_t)ws & 15)) return COFI_EWORKSPACE;
    hipStream_t s = cofi_s(stream);
    unsigned long long *keys = (unsigned long long *)ws;
    float *poses = (float *)((char *)ws + batch_key_bytes(rigs));
    if (hipError_t e = hipMemsetAsync(keys, 0, batch_key_bytes(rigs), s); e != hipSuccess) return (int)e;
    const RigOperands rig{BatchOperands{obj, img, count_dev, K_dev, obj_frame_stride, img_frame_stride, count_stride, coord_major ? 1 : 0, n_max},
                          ext_dev, ext_rig_stride, cameras};
    const float thr2 = reproj_err * reproj_err;
    const dim3 grid(cofi_cdiv(iterations, HPW * BATCH_WAVES), rigs), block(64 * BATCH_WAVES);
    const size_t lds = (size_t)n_max * 5 * sizeof(float);   // one camera's rows at a time: the batched kernel's footprint for any C
    if (lds <= 64 * 1024)   // by the capacity alone, never by device-side counts
        hipLaunchKernelGGL(pnp_hypotheses_rig_kernel<true>, grid, block, lds, s, rig, iterations, thr2, seed, poses, keys);
    else
        hipLaunchKernelGGL(pnp_hypotheses_rig_kernel<false>, grid, block, 0, s, rig, iterations, thr2, seed, poses, keys);
    hipLaunchKernelGGL(pnp_refine_rig_kernel, dim3(rigs), dim3(256), 0, s, rig, iterations, thr2, poses, keys, refine_iters, rig_pose,
                       rig_result, pose, result, inlier_mask);
    return cofi_launch_status();
}

extern "C" int cofi_pose_errors(const float *pose, const void *P_gt, int gt_is_f64, int frames, double *out, cofi_stream_t stream) {
    if (!pose || !P_gt || !out || frames <= 0) return COFI_EINVAL;
    hipStream_t s = cofi_s(stream);
    if (gt_is_f64)
        hipLaunchKernelGGL(pose_errors_kernel<double>, dim3(cofi_cdiv(frames, 64)), dim3(64), 0, s, pose, (const double *)P_gt, frames, out);
    else
        hipLaunchKernelGGL(pose_errors_kernel<float>, dim3(cofi_cdiv(frames, 64)), dim3(64), 0, s, pose, (const float *)P_gt, frames, out);
    return cofi_launch_status();
}

extern "C" int cofi_pose_covariance(const float *obj, const float *img, const int32_t *count_dev, int n_max, float fx, float fy, float cx,
                                    float cy, const float *pose, const int32_t *result, const uint8_t *inlier_mask, float sigma_px, double *cov,
                                    double *info, double *stat, cofi_stream_t stream) {
    if (!obj || !img || !pose || !result || !inlier_mask || !cov || !info || !stat || n_max <= 0 || !(fx > 0.f) || !(fy > 0.f) ||
        !(sigma_px == sigma_px))
        return COFI_EINVAL;
    hipLaunchKernelGGL(pose_covariance_kernel, dim3(1), dim3(64), 0, cofi_s(stream), obj, img, count_dev, n_max, Cam{fx, fy, cx, cy}, pose, result,
                       inlier_mask, sigma_px, cov, info, stat);
    return cofi_launch_status();
}

extern "C" int cofi_pose_covariance_batch(const float *obj, int obj_frame_stride, const float *img, int img_frame_stride, int coord_major,
                                          const int32_t *count_dev, int count_stride, const float *K_dev, int n_max, int frames,
                                          const float *pose, const int32_t *result, const uint8_t *inlier_mask, float sigma_px, double *cov,
                                          double *info, double *stat, cofi_stream_t stream) {
    if (!obj || !img || !K_dev || !pose || !result || !inlier_mask || !cov || !info || !stat || n_max <= 0 || frames <= 0 || frames > 65535 ||
        obj_frame_stride < 3 * n_max || img_frame_stride < 2 * n_max || (count_dev && count_stride < 1) || !(sigma_px == sigma_px))
        return COFI_EINVAL;
    const BatchOperands op{obj, img, count_dev, K_dev, obj_frame_stride, img_frame_stride, count_stride, coord_major ? 1 : 0, n_max};
    hipLaunchKernelGGL(pose_covariance_batch_kernel, dim3(cofi_cdiv(frames, COV_WAVES)), dim3(64 * COV_WAVES), 0, cofi_s(stream), op, frames, pose,
                       result, inlier_mask, sigma_px, cov, info, stat);
    return cofi_launch_status();
}

extern "C" int cofi_pose_covariance_rig(const float *obj, int obj_frame_stride, const float *img, int img_frame_stride, int coord_major,
                                        const int32_t *count_dev, int count_stride, const float *K_dev, const float *ext_dev, int ext_rig_stride,
                                        int n_max, int cameras, int rigs, const float *rig_pose, const int32_t *rig_result,
                                        const uint8_t *inlier_mask, float sigma_px, double *cov, double *info, double *stat,
                                        cofi_stream_t stream) {
    if (!obj || !img || !K_dev || !ext_dev || !rig_pose || !rig_result || !inlier_mask || !cov || !info || !stat || n_max <= 0 || cameras <= 0 ||
        rigs <= 0 || (long long)rigs * cameras > 65535 || obj_frame_stride < 3 * n_max || img_frame_stride < 2 * n_max ||
        (count_dev && count_stride < 1) || (ext_rig_stride != 0 && ext_rig_stride < 12 * cameras) || !(sigma_px == sigma_px))
        return COFI_EINVAL;
    const RigOperands rig{BatchOperands{obj, img, count_dev, K_dev, obj_frame_stride, img_frame_stride, count_stride, coord_major ? 1 : 0, n_max},
                          ext_dev, ext_rig_stride, cameras};
    hipLaunchKernelGGL(pose_covariance_rig_kernel, dim3(cofi_cdiv(rigs, COV_WAVES)), dim3(64 * COV_WAVES), 0, cofi_s(stream), rig, rigs, rig_pose,
                       rig_result, inlier_mask, sigma_px, cov, info, stat);
    return cofi_launch_status();
}

extern "C" int cofi_pose_nees(const float *pose, const void *P_gt, int gt_is_f64, const double *info, const double *stat, int frames,
                              double *nees, cofi_stream_t stream) {
    if (!pose || !P_gt || !info || !stat || !nees || frames <= 0) return COFI_EINVAL;
    hipStream_t s = cofi_s(stream);
    if (gt_is_f64)
        hipLaunchKernelGGL(pose_nees_kernel<double>, dim3(cofi_cdiv(frames, 64)), dim3(64), 0, s, pose, (const double *)P_gt, info, stat, frames,
                           nees);
    else
        hipLaunchKernelGGL(pose_nees_kernel<float>, dim3(cofi_cdiv(frames, 64)), dim3(64), 0, s, pose, (const float *)P_gt, info, stat, frames, nees);
    return cofi_launch_status();
}
