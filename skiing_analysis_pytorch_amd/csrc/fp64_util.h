// Scalar helpers of the float64 solver kernels (resect, refine, essential, person, scene, fuse, kinematics, evaluate):
// the finiteness tests, NaN-keeping maximum, 3-vector products, the confidence clamp, the order-preserving integer keys
// of the exact selections and NumPy's percentile position.  These kernels are bit-exact by rule, so each helper exists
// once: a change here changes every kernel the same way.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace skimi {

__host__ __device__ inline bool is_fin(double x) { return fabs(x) <= 1.79769313486231570815e308; }
__device__ inline bool fin3(const double* x) { return is_fin(x[0]) && is_fin(x[1]) && is_fin(x[2]); }
__host__ __device__ inline double qnan() { return __builtin_nan(""); }
// max that keeps a NaN, as NumPy's max does (fmax drops it)
__device__ inline double max_nan(double a, double b) { return (a != a || b != b) ? qnan() : fmax(a, b); }

__device__ inline double norm3(double a, double b, double c) { return sqrt(a * a + b * b + c * c); }
__device__ inline double dot3(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
__device__ inline void cross3(const double* a, const double* b, double* c) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

// a keypoint's confidence as a weight: clipped to [0, 1], 0 where it is not finite
__device__ inline double clamp_conf(double w) { return is_fin(w) ? fmin(fmax(w, 0.0), 1.0) : 0.0; }

// monotone map float -> uint32 (a < b as floats  <=>  key32(a) < key32(b) as unsigned; -0.0 sorts just below +0.0)
__device__ inline unsigned key32(float z) {
    const unsigned u = __float_as_uint(z);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ inline float unkey32(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }
// monotone map double -> uint64 (-0.0 just below +0.0, +-inf ordered)
__device__ inline unsigned long long key64(double x) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(x);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ULL);
}
__device__ inline double unkey64(unsigned long long k) {
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffULL) : ~k));
}

// NumPy's `linear` percentile on m >= 1 sorted values, in float64: v = q / 100 (m - 1), i = floor(v), gamma = v - i
struct PctPos {
    unsigned i0, i1;
    double gamma;
};
__device__ inline PctPos pct_pos(double q, unsigned m) {
    const double v = q / 100.0 * (double)(m - 1);
    const double fl = floor(v);
    PctPos p;
    p.i0 = (unsigned)fl;
    p.i1 = min(p.i0 + 1u, m - 1u);
    p.gamma = v - fl;
    return p;
}
__device__ inline double pct_lerp(double lo, double hi, double g) {
    const double d = hi - lo;
    return g < 0.5 ? lo + d * g : hi - d * (1.0 - g);
}

}  // namespace skimi
