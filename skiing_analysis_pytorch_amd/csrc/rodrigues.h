// Rodrigues' formula with a Taylor branch at small angles, shared by the bundle adjustment (ba.hip), the camera
// resection (resect.hip) and the camera-and-points refinement (refine.hip).  float64, device only.
#pragma once
#include <math.h>

namespace skimi {

constexpr double kSmallAngle2 = 1e-8;               // theta^2 below this: Taylor branch of Exp

// Rodrigues: E = I + A K + B K^2, K = [w]x, A = sin(th)/th, B = (1 - cos(th))/th^2; below kSmallAngle2 the Taylor
// polynomials in s = th^2.  a1 = A'(th)/th, b1 = B'(th)/th (the w-derivatives are a1 w_k, b1 w_k).
struct Rot {
    double A, B, a1, b1, Kx[9], K2[9];
};
__device__ inline void rodrigues(const double* w, Rot& r) {
    const double s = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
    if (s < kSmallAngle2) {
        r.A = 1.0 - s / 6.0 + s * s / 120.0;
        r.B = 0.5 - s / 24.0 + s * s / 720.0;
        r.a1 = -1.0 / 3.0 + s / 30.0;
        r.b1 = -1.0 / 12.0 + s / 180.0;
    } else {
        const double th = sqrt(s), sn = sin(th), cs = cos(th);
        r.A = sn / th;
        r.B = (1.0 - cs) / s;
        r.a1 = (th * cs - sn) / (s * th);
        r.b1 = (th * sn - 2.0 * (1.0 - cs)) / (s * s);
    }
    const double K[9] = {0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0};
#pragma unroll
    for (int k = 0; k < 9; ++k) r.Kx[k] = K[k];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) r.K2[i * 3 + j] = K[i * 3] * K[j] + K[i * 3 + 1] * K[3 + j] + K[i * 3 + 2] * K[6 + j];
}

// R = Exp(w) R0
__device__ inline void rotate(const Rot& r, const double* R0, double* R) {
    double E[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) E[k] = ((k % 4 == 0) ? 1.0 : 0.0) + r.A * r.Kx[k] + r.B * r.K2[k];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) R[i * 3 + j] = E[i * 3] * R0[j] + E[i * 3 + 1] * R0[3 + j] + E[i * 3 + 2] * R0[6 + j];
}

}  // namespace skimi
