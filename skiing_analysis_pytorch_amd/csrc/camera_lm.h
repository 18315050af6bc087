// The camera model shared by the Levenberg-Marquardt solvers of the camera resection (resect.hip) and the camera-and-points
// refinement (refine.hip): the projection with its weighted residual and the packing of a symmetric 6 x 6.  float64, device
// only.  Not here, and written in both files: rule 1's mask and weight load and the soft-L1 loss (resect.hip: load_point
// and inline in its two passes; refine.hip: point_used / load_obs, rho1_of / summand_change).  Merging them changes
// resect.hip's device assembly; profiles/shared_device_helpers.md.
#pragma once
#include "fp64_util.h"

namespace skimi {

// q = R X, the camera point's depth and ray, and the weighted residual with the principal point folded into the keypoint.
// Cam has R[9], t[3] and K[5] = fx, skew, cx, fy, cy.
struct Proj {
    double q[3], z, u, v, pu, r[2];
};
template <class Cam>
__device__ inline void residual(const Cam& s, const double* X, const double* x, double w, Proj& p) {
#pragma unroll
    for (int k = 0; k < 3; ++k) p.q[k] = s.R[3 * k] * X[0] + s.R[3 * k + 1] * X[1] + s.R[3 * k + 2] * X[2];
    p.z = p.q[2] + s.t[2];
    p.u = (p.q[0] + s.t[0]) / p.z;
    p.v = (p.q[1] + s.t[1]) / p.z;
    p.pu = s.K[0] * p.u + s.K[1] * p.v;
    p.r[0] = w * (p.pu + (s.K[2] - x[0]));
    p.r[1] = w * (s.K[3] * p.v + (s.K[4] - x[1]));
}

// index of (i, j) in a symmetric 6 x 6 packed by rows of the upper triangle
__device__ constexpr int packed(int i, int j) { return i <= j ? i * 6 - i * (i - 1) / 2 + (j - i) : j * 6 - j * (j - 1) / 2 + (i - j); }

}  // namespace skimi
