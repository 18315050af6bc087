// Fixed-order reductions of the float64 solver kernels.  Two schemes, which give different bits and are not to be mixed:
//  - wave_sum: a xor butterfly over the 64 lanes; every lane gets the same bits (a + b == b + a).  Overloads beside
//    common.h's float one.  wave_argmin: the same butterfly on a (value, index) pair (lsap.h: the next column of a path).
//  - block_sum / total / block_max: a shuffle-down tree per wave into `red`, then the waves in order.
#pragma once
#include "common.h"
#include "fp64_util.h"

namespace skimi {

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ unsigned wave_sum(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (unsigned)__shfl_xor((int)v, o, 64);
    return v;
}

// The smallest (value, index) pair of the 64 lanes, ordered by value and then by index: a xor butterfly, so every lane gets
// the same pair as long as no value is NaN (the order is then total and the minimum is one pair, or equal pairs).
__device__ __forceinline__ void wave_argmin(double& v, int& i) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(v, o, 64);
        const int oi = __shfl_xor(i, o, 64);
        if (ov < v || (ov == v && oi < i)) v = ov, i = oi;
    }
}

// Exact selection of two ranks by one wave: the keys (order-preserving, key64) are spread over the lanes, for_keys(f) calls
// f(key) for each of the calling lane's keys, k0 <= k1 are 0-based ranks below the number of keys.  64 passes from the top
// bit down: count the keys that agree with the prefix above the bit and have the bit clear (wave_sum: every lane gets the
// same count), then step past them or stay.  p0, p1: the keys of rank k0, k1, the same in every lane.  The two middle
// ranks (n - 1) / 2, n / 2 give a median (evaluate.hip: per-joint error tables; fuse.hip: bone lengths over a clip).
template <class ForKeys>
__device__ inline void wave_select2(unsigned k0, unsigned k1, ForKeys&& for_keys, unsigned long long& p0, unsigned long long& p1) {
    p0 = p1 = 0;
    for (int bit = 63; bit >= 0; --bit) {
        unsigned c0 = 0, c1 = 0;
        for_keys([&](unsigned long long key) {
            c0 += ((key ^ p0) >> bit) == 0;    // the bits above agree with the prefix and this one is 0
            c1 += ((key ^ p1) >> bit) == 0;
        });
        c0 = wave_sum(c0), c1 = wave_sum(c1);
        if (k0 >= c0) k0 -= c0, p0 |= 1ULL << bit;
        if (k1 >= c1) k1 -= c1, p1 |= 1ULL << bit;
    }
}

// fixed-order workgroup sums of N values per thread: a shuffle tree inside each wave, then `total` adds the waves in
// order, so every thread that reads total k gets the same bits.  The caller alternates `red` between two buffers: one
// barrier per reduction suffices, and a total stays readable until the next-but-one reduction.
template <int N, int kRed>
__device__ inline void block_sum(const double (&v)[N], double (*red)[kRed]) {
    static_assert(N <= kRed, "red holds kRed sums per wave");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        double x = v[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o, 64);
        if (lane == 0) red[wave][k] = x;
    }
    __syncthreads();
}
// kWaves: the workgroup's wave count where it is a constant (the compiler unrolls the sum), 0 to read it from the launch
template <int kWaves = 0, int kRed>
__device__ inline double total(const double (*red)[kRed], int k) {
    const int waves = kWaves > 0 ? kWaves : (int)(blockDim.x >> 6);
    double s = red[0][k];
    for (int w = 1; w < waves; ++w) s += red[w][k];
    return s;
}
// a workgroup maximum (which does not depend on the order); readable by thread 0 after the call
__device__ inline double block_max(double x, double* smax, bool keep_nan) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double y = __shfl_down(x, o, 64);
        x = keep_nan ? max_nan(x, y) : fmax(x, y);
    }
    __syncthreads();                           // the last reader of smax is done
    if ((threadIdx.x & 63) == 0) smax[threadIdx.x >> 6] = x;
    __syncthreads();
    double m = smax[0];
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w) m = keep_nan ? max_nan(m, smax[w]) : fmax(m, smax[w]);
    return m;
}

}  // namespace skimi
