// The 3 x 3 polar factor by one-sided Jacobi, shared by the fusion (fuse.hip) and the Procrustes error (evaluate.hip).
#pragma once
#include <math.h>

#include "fp64_util.h"

namespace skimi {

constexpr int kSvd3Sweeps = 40;

// A (row-major 3 x 3) = U S V^T by one-sided Jacobi on the columns -> Q = u1 v1^T + u2 v2^T + (u1 x u2)(v1 x v2)^T over the
// two largest singular values, and ssum = the sum of the three.  Q is the polar factor U V^T with the singular vector of
// the smallest singular value flipped when det(U V^T) < 0: what the reference's "flip the last column" produces, whatever
// signs its SVD chose.  A zero third column (a 3 x 2 problem) is never rotated and comes out as the smallest.  s_min is the
// smallest singular value and det_sign the sign of det(U V^T) before that flip (+1 where s_min is 0).
__device__ inline void polar3_signed(const double* A, double* Q, double& ssum, double& s_min, double& det_sign) {
    double a[3][3], v[3][3];                   // [column][row]
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            a[c][r] = A[3 * r + c];
            v[c][r] = r == c ? 1.0 : 0.0;
        }
    for (int sweep = 0; sweep < kSvd3Sweeps; ++sweep) {
        bool rotated = false;
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int q = p + 1; q < 3; ++q) {
                const double al = a[p][0] * a[p][0] + a[p][1] * a[p][1] + a[p][2] * a[p][2];
                const double be = a[q][0] * a[q][0] + a[q][1] * a[q][1] + a[q][2] * a[q][2];
                const double ga = a[p][0] * a[q][0] + a[p][1] * a[q][1] + a[p][2] * a[q][2];
                if (fabs(ga) > 1e-15 * sqrt(al * be)) {
                    rotated = true;
                    const double zeta = (be - al) / (2.0 * ga);
                    const double tn = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(zeta * zeta + 1.0));
                    const double cs = 1.0 / sqrt(tn * tn + 1.0), sn = tn * cs;
#pragma unroll
                    for (int r = 0; r < 3; ++r) {
                        const double ap = a[p][r], aq = a[q][r], vp = v[p][r], vq = v[q][r];
                        a[p][r] = cs * ap - sn * aq;
                        a[q][r] = sn * ap + cs * aq;
                        v[p][r] = cs * vp - sn * vq;
                        v[q][r] = sn * vp + cs * vq;
                    }
                }
            }
        if (!rotated) break;
    }
    double sg[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) sg[c] = norm3(a[c][0], a[c][1], a[c][2]);
    ssum = sg[0] + sg[1] + sg[2];
    const int k = (sg[0] <= sg[1] && sg[0] <= sg[2]) ? 0 : (sg[1] <= sg[2] ? 1 : 2);      // the smallest
    double u1[3], u2[3], v1[3], v2[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double s1 = k == 0 ? sg[1] : k == 1 ? sg[2] : sg[0], s2 = k == 0 ? sg[2] : k == 1 ? sg[0] : sg[1];
        u1[r] = (k == 0 ? a[1][r] : k == 1 ? a[2][r] : a[0][r]) / s1;
        u2[r] = (k == 0 ? a[2][r] : k == 1 ? a[0][r] : a[1][r]) / s2;
        v1[r] = k == 0 ? v[1][r] : k == 1 ? v[2][r] : v[0][r];
        v2[r] = k == 0 ? v[2][r] : k == 1 ? v[0][r] : v[1][r];
    }
    const double u3[3] = {u1[1] * u2[2] - u1[2] * u2[1], u1[2] * u2[0] - u1[0] * u2[2], u1[0] * u2[1] - u1[1] * u2[0]};
    const double v3[3] = {v1[1] * v2[2] - v1[2] * v2[1], v1[2] * v2[0] - v1[0] * v2[2], v1[0] * v2[1] - v1[1] * v2[0]};
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) Q[3 * r + c] = u1[r] * v1[c] + u2[r] * v2[c] + u3[r] * v3[c];
    // det(U V^T) of the unflipped factors: the smallest pair (a_k / s_k, v_k) against the completed one (u3, v3)
    double du = 0.0, dv = 0.0;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        du += u3[r] * (k == 0 ? a[0][r] : k == 1 ? a[1][r] : a[2][r]);
        dv += v3[r] * (k == 0 ? v[0][r] : k == 1 ? v[1][r] : v[2][r]);
    }
    s_min = k == 0 ? sg[0] : k == 1 ? sg[1] : sg[2];
    det_sign = ((du < 0.0) != (dv < 0.0)) ? -1.0 : 1.0;
}

__device__ inline void polar3(const double* A, double* Q, double& ssum) {
    double s_min, sign;
    polar3_signed(A, Q, ssum, s_min, sign);
}

}  // namespace skimi
