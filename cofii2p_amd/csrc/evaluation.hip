// The evaluation pass of the reference on the device: per frame of a stack-mode submission, what evaluation/eval_all.py:107-117 keeps
// of the pose (success, RTE, RRE) and what evaluation/IR_RMSE.py:36-59 computes from the frame's result file (the mean reprojection
// residual against the ground-truth pose and the number of residuals under every pixel threshold) - one launch, one workgroup per
// frame, operands read in place as cofi_match_finish and cofi_pnp_ransac_batch leave them, no host read: capturable in a hipGraph.
// Everything is fp64 without contraction.  The residual sum is taken in an order that depends on the frame's count only (thread t adds
// residuals t, t + 256, ... in ascending order, then a fixed butterfly per wave and a fixed tree over the four waves), so a frame's row
// does not depend on the batch it is in.  The counts are integers: lane t of a wave counts threshold t from ballots.
#include "pose_errors.h"

namespace {

constexpr int EVAL_NT = 256, EVAL_NW = EVAL_NT / 64, EVAL_MAXT = 64, EVAL_COLS = 6;

struct EvalArgs {
    const float *obj;          // frame f: obj + f * obj_stride, (n_max, 3)
    const float *img;          // frame f: img + f * img_stride; (n_max, 2), or (2, n_max) if coord_major
    const int32_t *count;      // frame f: count[f * count_stride] valid rows (NULL: n_max)
    const float *K;            // (frames, 3, 3) row-major
    const float *pose;         // (frames, 12)
    const int32_t *result;     // (frames, 3)
    const double *thresholds;  // (T)
    const int32_t *row_index;  // (frames)
    double *rows;              // (table_rows, 6 + T)
    int obj_stride, img_stride, count_stride, coord_major, n_max, T, table_rows;
};

template <class G>
__global__ __launch_bounds__(EVAL_NT) void eval_monitors_kernel(EvalArgs a, const G *P_gt) {
    __shared__ double s_thr[EVAL_MAXT];
    __shared__ double s_sum[EVAL_NW];
    __shared__ int s_cnt[EVAL_NW][EVAL_MAXT];
    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int row = a.row_index[f];
    if (row < 0 || row >= a.table_rows) return;   // a padding frame (or an index outside the table): nothing is written
    int n = a.count ? a.count[(size_t)f * a.count_stride] : a.n_max;
    n = n < 0 ? 0 : (n > a.n_max ? a.n_max : n);
    if (tid < a.T) s_thr[tid] = a.thresholds[tid];
    __syncthreads();

    const G *P = P_gt + 16 * (size_t)f;
    double R[9], t[3], Km[9];
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) {
            R[3 * r + c] = (double)P[4 * r + c];
            Km[3 * r + c] = (double)a.K[9 * (size_t)f + 3 * r + c];
        }
        t[r] = (double)P[4 * r + 3];
    }
    const float *X = a.obj + (size_t)f * a.obj_stride;
    const float *uv = a.img + (size_t)f * a.img_stride;
    const float *pu = uv, *pv = a.coord_major ? uv + a.n_max : uv + 1;
    const int step = a.coord_major ? 1 : 2;

    double acc = 0.0;
    int cnt = 0;   // lane t: residuals of this wave's points <= thresholds[t]
    for (int base = wv * 64; base < n; base += EVAL_NT) {   // wave-uniform: the ballots below see whole waves
        const int i = base + lane;
        const bool valid = i < n;
        double res = 0.0;
        if (valid) {
            const double x = (double)X[3 * (size_t)i], y = (double)X[3 * (size_t)i + 1], z = (double)X[3 * (size_t)i + 2];
            double cam[3], proj[3];
            for (int r = 0; r < 3; ++r) cam[r] = ((R[3 * r] * x + R[3 * r + 1] * y) + R[3 * r + 2] * z) + t[r];
            for (int r = 0; r < 3; ++r) proj[r] = (Km[3 * r] * cam[0] + Km[3 * r + 1] * cam[1]) + Km[3 * r + 2] * cam[2];
            const double du = (double)pu[(size_t)i * step] - proj[0] / proj[2], dv = (double)pv[(size_t)i * step] - proj[1] / proj[2];
            res = sqrt(du * du + dv * dv);
            acc += res;
        }
        for (int k = 0; k < a.T; ++k) {
            const unsigned long long b = __ballot(valid && res <= s_thr[k]);   // a NaN residual compares false
            if (lane == k) cnt += __popcll(b);
        }
    }
    const double wsum = wave_sum_d(acc);
    if (lane == 0) s_sum[wv] = wsum;
    s_cnt[wv][lane] = cnt;
    __syncthreads();

    double *out = a.rows + (size_t)row * (EVAL_COLS + a.T);
    if (tid < a.T) out[EVAL_COLS + tid] = (double)((s_cnt[0][tid] + s_cnt[1][tid]) + (s_cnt[2][tid] + s_cnt[3][tid]));
    if (tid == 0) {
        const int success = a.result[3 * (size_t)f];
        out[0] = (double)n;
        out[1] = (double)success;
        out[2] = (double)a.result[3 * (size_t)f + 1];
        double rte = __builtin_nan(""), rre = __builtin_nan("");
        if (success != 0) pose_errors_frame(a.pose + 12 * (size_t)f, P, &rte, &rre);
        out[3] = rte;
        out[4] = rre;
        out[5] = n > 0 ? ((s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3])) / (double)n : __builtin_nan("");
    }
}

}  // namespace

extern "C" int cofi_eval_monitors(const float *obj, int obj_frame_stride, const float *img, int img_frame_stride, int coord_major,
                                  const int32_t *count_dev, int count_stride, const float *K_dev, int n_max, int frames, const float *pose,
                                  const int32_t *result, const void *P_gt, int gt_is_f64, const double *thresholds, int T,
                                  const int32_t *row_index, double *rows, int table_rows, cofi_stream_t stream) {
    if (!obj || !img || !K_dev || !pose || !result || !P_gt || !thresholds || !row_index || !rows || n_max <= 0 || frames <= 0 || T < 1 ||
        table_rows <= 0 || obj_frame_stride < 3 * n_max || img_frame_stride < 2 * n_max || (count_dev && count_stride < 1))
        return COFI_EINVAL;
    if (T > EVAL_MAXT) return COFI_EUNSUPPORTED;
    const EvalArgs a{obj, img, count_dev, K_dev, pose, result, thresholds, row_index, rows, obj_frame_stride, img_frame_stride,
                     count_stride, coord_major ? 1 : 0, n_max, T, table_rows};
    hipStream_t s = cofi_s(stream);
    if (gt_is_f64)
        hipLaunchKernelGGL(eval_monitors_kernel<double>, dim3(frames), dim3(EVAL_NT), 0, s, a, (const double *)P_gt);
    else
        hipLaunchKernelGGL(eval_monitors_kernel<float>, dim3(frames), dim3(EVAL_NT), 0, s, a, (const float *)P_gt);
    return cofi_launch_status();
}
