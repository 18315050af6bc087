// The person-centred world origin of the clip path, on device so the dense world-point maps never leave HBM:
//   person origin of a point map   (extract_person_points + its caller's mean, vggt/multi_view_process.py:356-395,
//                                   :195-199): crop to the detector box, keep the finite points, keep those within
//                                   3 sigma of the median depth, average them
//   recentre + align the cameras   (:201-217): t_c += R_c origin, and at two views the right camera's 180-degree turn
// Rules where NumPy's float32 result depends on its implementation: DESIGN §2 "Person origin".
//
// One workgroup per map, one launch, no cross-workgroup combine.  The median is an exact selection: a radix select over
// the order-preserving 32-bit key of z, four passes of an 8-bit LDS histogram.  Every floating-point sum has a fixed
// order (a thread adds its strided elements in index order, the waves' shuffle trees and the in-order sum of the waves
// follow); counts and histograms use integer LDS atomics, whose result does not depend on order.
#include <math.h>

#include "common.h"
#include "fp64_util.h"

namespace skimi {

constexpr int kPersonThreads = 1024;
constexpr int kPersonWaves = kPersonThreads / 64;

// the box of `extract_person_points` (:364-383) in map pixels: products in float64, truncation toward zero, clip
struct Crop {
    int x1, y1, w, h;   // w or h <= 0: empty
};

__device__ inline int trunc_to_int(double v) {   // Python's int(); a non-finite product gives an empty box instead of raising
    if (!(fabs(v) < 1e9)) return v > 0 ? 1000000000 : (v < 0 ? -1000000000 : 0);
    return (int)v;
}

__device__ inline Crop crop_of(const float* box, int H, int W, double src_h, double src_w) {
    const double sx = (double)W / src_w, sy = (double)H / src_h;
    Crop c;
    const bool finite = isfinite(box[0]) && isfinite(box[1]) && isfinite(box[2]) && isfinite(box[3]);
    int x1 = trunc_to_int((double)box[0] * sx), x2 = trunc_to_int((double)box[2] * sx);
    int y1 = trunc_to_int((double)box[1] * sy), y2 = trunc_to_int((double)box[3] * sy);
    x1 = min(max(x1, 0), W - 1);
    x2 = min(max(x2, 0), W);
    y1 = min(max(y1, 0), H - 1);
    y2 = min(max(y2, 0), H);
    c.x1 = x1;
    c.y1 = y1;
    c.w = finite ? x2 - x1 : 0;
    c.h = finite ? y2 - y1 : 0;
    return c;
}

// one histogram increment per lane; a wave whose active lanes all hit one bin (the usual case of the first passes: the
// depths of a person share their exponent) adds its lane count once instead of serialising 64 atomics on one address
__device__ inline void hist_add(unsigned* hist, unsigned bin, bool active) {
    const unsigned long long mask = __ballot(active);
    if (mask == 0) return;
    const int leader = __ffsll((long long)mask) - 1;
    const unsigned first = __shfl((int)bin, leader, 64);
    if (__all(!active || bin == first)) {
        if ((int)(threadIdx.x & 63) == leader) atomicAdd(&hist[first], (unsigned)__popcll(mask));
    } else if (active) {
        atomicAdd(&hist[bin], 1u);
    }
}

// fixed-order workgroup sum of N doubles per thread -> every thread gets the same bits
template <int N>
__device__ inline void block_sum(double (&v)[N], double (*red)[4]) {
    static_assert(N <= 4, "red holds four sums per wave");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();   // `red` may still be read from the previous reduction
#pragma unroll
    for (int k = 0; k < N; ++k) {
        double x = v[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o, 64);
        if (lane == 0) red[wave][k] = x;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; ++k) {
        double s = red[0][k];
        for (int w = 1; w < kPersonWaves; ++w) s += red[w][k];
        v[k] = s;
    }
}

// stats [M, 8] = n_box, n_valid, n_kept, median, std, origin x, y, z
__global__ __launch_bounds__(kPersonThreads) void person_origin_kernel(const float* __restrict__ points,
                                                                       const float* __restrict__ boxes, int H, int W,
                                                                       double src_h, double src_w,
                                                                       double* __restrict__ stats) {
    __shared__ unsigned hist[256];
    __shared__ double red[kPersonWaves][4];
    __shared__ unsigned s_prefix, s_rank, s_below, s_equal, s_above;
    const int m = blockIdx.x, tid = threadIdx.x;
    const Crop c = crop_of(boxes + (long)m * 4, H, W, src_h, src_w);
    double* out = stats + (long)m * 8;
    const long n_box = (c.w > 0 && c.h > 0) ? (long)c.w * c.h : 0;
    const float* base = points + (long)m * H * W * 3;
    const double nan = qnan();
    if (n_box == 0) {
        if (tid == 0) {
            out[0] = 0; out[1] = 0; out[2] = 0; out[3] = nan; out[4] = nan; out[5] = nan; out[6] = nan; out[7] = nan;
        }
        return;
    }
    // element i of the crop, row-major as pointmap[y1:y2, x1:x2].reshape(-1, 3)
    auto at = [&](long i) {   // n_box < 2^28: 32-bit division
        const int r = (int)i / c.w;
        return base + ((long)(c.y1 + r) * W + (c.x1 + ((int)i - r * c.w))) * 3;
    };
    auto valid = [](const float* p) { return isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]); };

    // pass 1: valid count, sum of z (the mean), histogram of the key's top byte
    if (tid < 256) hist[tid] = 0;
    __syncthreads();
    double acc[4] = {0, 0, 0, 0};
    for (long i0 = 0; i0 < n_box; i0 += kPersonThreads) {
        const long i = i0 + tid;
        bool ok = false;
        unsigned bin = 0;
        if (i < n_box) {
            const float* p = at(i);
            ok = valid(p);
            if (ok) {
                acc[0] += 1.0;
                acc[1] += (double)p[2];
                bin = key32(p[2]) >> 24;
            }
        }
        hist_add(hist, bin, ok);
    }
    block_sum(acc, red);
    const long n = (long)acc[0];   // exact: a sum of at most 2^31 ones
    if (n == 0) {
        if (tid == 0) {
            out[0] = (double)n_box; out[1] = 0; out[2] = 0; out[3] = nan; out[4] = nan; out[5] = nan; out[6] = nan; out[7] = nan;
        }
        return;
    }
    const double mean = acc[1] / (double)n;
    // the lower middle order statistic has 0-based rank (n - 1) / 2; an even n also needs rank n / 2
    if (tid == 0) {
        s_prefix = 0;
        s_rank = (unsigned)((n - 1) / 2);
        s_below = 0;
    }
    double dev[1] = {0};
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        if (pass > 0) {
            // passes 2-4: histogram of the next byte among the keys that match the prefix; pass 2 also sums the
            // squared deviations from the mean
            const unsigned prefix = s_prefix;
            const unsigned hi_mask = 0xFFFFFFFFu << (shift + 8);
            for (long i0 = 0; i0 < n_box; i0 += kPersonThreads) {
                const long i = i0 + tid;
                bool hit = false;
                unsigned bin = 0;
                if (i < n_box) {
                    const float* p = at(i);
                    if (valid(p)) {
                        const unsigned k = key32(p[2]);
                        hit = (k & hi_mask) == prefix;
                        bin = (k >> shift) & 255u;
                        if (pass == 1) {
                            const double d = (double)p[2] - mean;
                            dev[0] += d * d;
                        }
                    }
                }
                hist_add(hist, bin, hit);
            }
        }
        __syncthreads();
        if (tid == 0) {   // the bin that holds the rank; 256 adds
            unsigned r = s_rank, b = 0;
            while (b < 255 && r >= hist[b]) r -= hist[b++];
            s_below += s_rank - r;
            s_rank = r;
            s_prefix |= b << shift;
            s_equal = hist[b];
        }
        __syncthreads();
        if (tid < 256) hist[tid] = 0;
        __syncthreads();
    }
    block_sum(dev, red);
    const double sd = sqrt(dev[0] / (double)n);
    const unsigned lower = s_prefix;
    double median = (double)unkey32(lower);
    if ((n & 1) == 0) {
        // upper middle (rank n / 2): the lower one again if count(key <= lower) > n / 2, else the smallest key above it
        unsigned upper = lower;
        if (!((long)s_below + (long)s_equal > n / 2)) {
            if (tid == 0) s_above = 0xFFFFFFFFu;
            __syncthreads();
            unsigned best = 0xFFFFFFFFu;
            for (long i = tid; i < n_box; i += kPersonThreads) {
                const float* p = at(i);
                if (valid(p)) {
                    const unsigned k = key32(p[2]);
                    if (k > lower && k < best) best = k;
                }
            }
            for (int o = 32; o > 0; o >>= 1) best = min(best, (unsigned)__shfl_xor((int)best, o, 64));
            if ((tid & 63) == 0) atomicMin(&s_above, best);
            __syncthreads();
            upper = s_above;
        }
        median = ((double)unkey32(lower) + (double)unkey32(upper)) / 2.0;   // exact: both are float32
    }
    // last pass: the points with |z - median| < 3 std (strict, float64) and their sum
    const double lim = 3.0 * sd;
    double kept[4] = {0, 0, 0, 0};
    for (long i = tid; i < n_box; i += kPersonThreads) {
        const float* p = at(i);
        if (valid(p) && fabs((double)p[2] - median) < lim) {
            kept[0] += 1.0;
            kept[1] += (double)p[0];
            kept[2] += (double)p[1];
            kept[3] += (double)p[2];
        }
    }
    block_sum(kept, red);
    if (tid == 0) {
        const double nk = kept[0];
        out[0] = (double)n_box;
        out[1] = (double)n;
        out[2] = nk;
        out[3] = median;
        out[4] = sd;
        out[5] = nk > 0 ? kept[1] / nk : nan;
        out[6] = nk > 0 ? kept[2] / nk : nan;
        out[7] = nk > 0 ? kept[3] / nk : nan;
    }
}

// One thread per time step: origin = float64 mean of the step's S person origins in view order (zero if any view kept
// nothing), t_c += R_c origin; at S = 2 view 1 is turned by diag(-1, 1, -1) (rows 0 and 2 of R_1 change sign) while
// t_1 keeps its value: the reference turns it and then mirrors x and z back (:214-218).
__global__ void recenter_cameras_kernel(const double* __restrict__ stats, const float* __restrict__ E, long steps, int S,
                                        double* __restrict__ origin_out, float* __restrict__ R_out,
                                        float* __restrict__ t_out) {
    const long s = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= steps) return;
    double o[3] = {0, 0, 0};
    bool all_kept = true;
    for (int v = 0; v < S; ++v) {
        const double* st = stats + (s * S + v) * 8;
        all_kept = all_kept && st[2] > 0;
        for (int k = 0; k < 3; ++k) o[k] += st[5 + k];
    }
    for (int k = 0; k < 3; ++k) o[k] = all_kept ? o[k] / (double)S : 0.0;
    for (int k = 0; k < 3; ++k) origin_out[s * 3 + k] = o[k];
    for (int v = 0; v < S; ++v) {
        const float* e = E + (s * S + v) * 12;
        float* R = R_out + (s * S + v) * 9;
        float* t = t_out + (s * S + v) * 3;
        for (int a = 0; a < 3; ++a) {
            double acc = (double)e[a * 4 + 3];
            double ro = 0;
            for (int b = 0; b < 3; ++b) ro += (double)e[a * 4 + b] * o[b];
            acc += ro;
            t[a] = (float)acc;
            const float sign = (S == 2 && v == 1 && a != 1) ? -1.0f : 1.0f;
            for (int b = 0; b < 3; ++b) R[a * 3 + b] = sign * e[a * 4 + b];
        }
    }
}

}  // namespace skimi

using namespace skimi;

extern "C" {

size_t skimi_person_workspace_bytes(int64_t maps, int32_t H, int32_t W) {
    (void)maps; (void)H; (void)W;
    return 0;   // one workgroup per map: nothing is combined across workgroups
}

int skimi_person_origin(const float* points, const float* boxes, int64_t maps, int32_t H, int32_t W, int32_t src_h,
                        int32_t src_w, void* workspace, double* stats, void* stream) {
    (void)workspace;
    SKIMI_CHECK_ARG(points && boxes && stats && maps > 0 && maps < ((int64_t)1 << 31) && H > 0 && W > 0 && src_h > 0 && src_w > 0 &&
                        (int64_t)H * W <= (int64_t)1 << 28,
                    "skimi_person_origin: bad arguments (need maps of at most 2^28 pixels, a positive source size)");
    hipLaunchKernelGGL(person_origin_kernel, dim3((unsigned)maps), dim3(kPersonThreads), 0, (hipStream_t)stream, points, boxes,
                       H, W, (double)src_h, (double)src_w, stats);
    SKIMI_LAUNCH_CHECK();
    return SKIMI_OK;
}

int skimi_recenter_cameras(const double* stats, const float* extrinsic, int64_t steps, int32_t views, double* origin_out,
                           float* R_out, float* t_out, void* stream) {
    SKIMI_CHECK_ARG(stats && extrinsic && origin_out && R_out && t_out && steps > 0 && views >= 1 && views <= 8,
                    "skimi_recenter_cameras: bad arguments (need 1..8 views)");
    hipLaunchKernelGGL(recenter_cameras_kernel, dim3((unsigned)cdiv(steps, 64)), dim3(64), 0, (hipStream_t)stream, stats,
                       extrinsic, (long)steps, views, origin_out, R_out, t_out);
    SKIMI_LAUNCH_CHECK();
    return SKIMI_OK;
}

}  // extern "C"
