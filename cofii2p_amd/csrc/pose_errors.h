// The registration errors of one pose (evaluation/eval_all.py:16-22) as a device function: the one body behind cofi_pose_errors
// (csrc/pnp.hip) and columns 3, 4 of cofi_eval_monitors (csrc/evaluation.hip).  Plain fp64 operations in a fixed order and libm calls
// (the library is built with -ffp-contract=off): the same inputs give the same bits in either kernel.
#pragma once
#include "common.h"

// pose: 12 floats (R row-major | t) of the predicted pose; P_gt: the 16 entries of the ground-truth matrix, row-major.
// P_diff = inv(P_pred) P_gt; *rte = |t(P_diff)|, *rre = sum |euler 'xzy' of R(P_diff)| in degrees; both NaN for a singular P_pred.
template <class T>
__device__ inline void pose_errors_frame(const float *pose, const T *P_gt, double *rte_out, double *rre_out) {
    // [P_pred | I] -> [I | inv(P_pred)]: Gauss-Jordan with partial pivoting, fp64.  A general inverse: the refit's R is orthonormal to fp32 only.
    double A[4][8];
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 8; ++c) A[r][c] = c < 4 ? (r == c ? 1.0 : 0.0) : (c - 4 == r ? 1.0 : 0.0);
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) A[r][c] = (double)pose[3 * r + c];
        A[r][3] = (double)pose[9 + r];
    }
    bool ok = true;
    for (int col = 0; col < 4; ++col) {
        int piv = col;
        for (int r = col + 1; r < 4; ++r)
            if (fabs(A[r][col]) > fabs(A[piv][col])) piv = r;
        if (!(fabs(A[piv][col]) > 0.0)) { ok = false; break; }
        if (piv != col)
            for (int j = 0; j < 8; ++j) { const double tmp = A[col][j]; A[col][j] = A[piv][j]; A[piv][j] = tmp; }
        const double d = A[col][col];
        for (int j = 0; j < 8; ++j) A[col][j] /= d;
        for (int r = 0; r < 4; ++r) {
            if (r == col) continue;
            const double fct = A[r][col];
            for (int j = 0; j < 8; ++j) A[r][j] -= fct * A[col][j];
        }
    }
    if (!ok) {   // singular P_pred: no error is defined
        *rte_out = *rre_out = __builtin_nan("");
        return;
    }
    double D[3][4];   // the three rows of P_diff the errors read
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 4; ++c) {
            double acc = 0.0;
            for (int k = 0; k < 4; ++k) acc += A[r][4 + k] * (double)P_gt[4 * k + c];
            D[r][c] = acc;
        }
    const double rte = sqrt(D[0][3] * D[0][3] + D[1][3] * D[1][3] + D[2][3] * D[2][3]);
    // scipy's as_euler('xzy') as pose.euler_xzy_deg restates it: R = Ry(c) Rz(b) Rx(a); gimbal lock: third angle zero
    const double s = D[1][0];
    const double b = asin(s > 1.0 ? 1.0 : (s < -1.0 ? -1.0 : s));
    double a, c;
    if (fabs(s) < 1.0 - 1e-12) {
        a = atan2(-D[1][2], D[1][1]);
        c = atan2(-D[2][0], D[0][0]);
    } else {
        a = atan2(D[2][1], D[2][2]);
        c = 0.0;
    }
    const double deg = 180.0 / 3.14159265358979323846;
    *rte_out = rte;
    *rre_out = fabs(a * deg) + fabs(b * deg) + fabs(c * deg);
}
