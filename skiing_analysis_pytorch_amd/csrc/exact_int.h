// Exact integer arithmetic carried in doubles, for the rasterisers (draw.hip, scene_view.hip).  Their coordinates are int32
// saturated to +-2^20 (1/16 pixel), so every difference is below 2^22 in size and every product, sum and root of the
// distance tests is an integer below 2^46, far inside the 2^53 a double holds exactly: each operation is exact (the build
// does not contract a b + c, and a contraction would change nothing here).  An f64 operation is one instruction on gfx950,
// a 64-bit integer multiply or divide a sequence of 32-bit ones.
#pragma once
#include "common.h"

namespace skimi {

constexpr int kSat = 1 << 20;                     // coordinates and radii, in 1/16 pixel

__device__ __forceinline__ int sat20(int v) { return min(max(v, -kSat), kSat); }

// exact floor square root of an integer 0 <= n < 2^52: the rounded root is within one of it
__device__ __forceinline__ double isqrt_exact(double n) {
    double r = floor(sqrt(n));
    if (r * r > n) r -= 1.0;
    if ((r + 1.0) * (r + 1.0) <= n) r += 1.0;
    return r;
}

// exact floor(c / m) of integers 0 <= c < 2^52, 1 <= m: the rounded quotient's floor is within one of it
__device__ __forceinline__ double floor_div_exact(double c, double m) {
    double q = floor(c / m);
    if (q * m > c) q -= 1.0;
    if ((q + 1.0) * m <= c) q += 1.0;
    return q;
}

}  // namespace skimi
