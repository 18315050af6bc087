// Point-to-plane ICP between two dense VGGT point maps (the refinement of the right camera in
// vggt/multi_view_process.py:263-291, ICP_with_bbox :427-520), without Open3D:
//   validity filter + order-preserving compaction of each cloud        (:463-474)
//   hashed uniform grid over the target, cells sorted by point index
//   radius-neighbourhood normals of the target, float64 cumulants       (estimate_normals, :487-496)
//   one kernel per iteration: transform, nearest neighbour, 6x6 system  (registration_icp, :498-505)
// The 6x6 solve, the Euler composition and the convergence test run on the host (api side of this file).
//
// Rules where Open3D's result depends on its implementation (DESIGN §2 "ICP"):
//   - a point is valid iff all three coordinates are finite and x^2 + y^2 + z^2 > 1e-12 (float64); the reference keeps
//     ||p|| > 1e-6 and differs only on non-finite input (an inf point would enter its clouds);
//   - a neighbour / correspondence is at d^2 < r^2, d^2 = dx*dx + dy*dy + dz*dz in float64 (the strict test of nanoflann);
//   - an equidistant correspondence goes to the target point with the smaller index;
//   - every sum is taken in a fixed order (no float atomics): results are bitwise reproducible;
//   - normals are the eigenvector of the smallest eigenvalue of the float64 covariance (cyclic Jacobi to convergence),
//     (0, 0, 1) below 3 neighbours; their sign is arbitrary and does not enter the point-to-plane system.
#include <math.h>

#include <algorithm>
#include <cmath>

#include "common.h"
#include "reduce.h"

namespace skimi {
namespace {

constexpr int kThreads = 256;
constexpr int kScanItems = 4;                     // elements per thread of the scan kernels
constexpr int kScanBlock = kThreads * kScanItems;
constexpr int kSums = 29;                         // 21 JtJ (upper triangle, row-major) + 6 Jtr + sum d^2 + count
constexpr int kSlab = 32;                         // stride of one workgroup's partials
constexpr int kCellClamp = (1 << 20) - 2;         // cell coordinates are clamped to +-kCellClamp
constexpr double kCellPad = 1.0001;               // cell edge = radius * kCellPad >= the largest search radius
constexpr int kMinPoints = 50;                    // multi_view_process.py:471-474

struct Mat34 {
    double m[12];
};

// ---- integer scans (exclusive; out[L] = total) ------------------------------------------------
__device__ int block_exclusive_scan(int v, int* total) {
    __shared__ int wsum[kThreads / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(inc, o, 64);
        if (lane >= o) inc += u;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kThreads / 64; ++w) {
        before += w < wave ? wsum[w] : 0;
        all += wsum[w];
    }
    __syncthreads();
    *total = all;
    return before + inc - v;
}

__global__ __launch_bounds__(kThreads) void scan_block_sums_kernel(const int* __restrict__ in, long L, int* __restrict__ blk) {
    const long base = (long)blockIdx.x * kScanBlock + threadIdx.x * kScanItems;
    int s = 0;
#pragma unroll
    for (int k = 0; k < kScanItems; ++k)
        if (base + k < L) s += in[base + k];
    int total;
    block_exclusive_scan(s, &total);
    if (threadIdx.x == 0) blk[blockIdx.x] = total;
}

// one workgroup: blk[0..nb) -> exclusive offsets, blk[nb] = total
__global__ __launch_bounds__(kThreads) void scan_top_kernel(int* __restrict__ blk, int nb) {
    const int per = (nb + kThreads - 1) / kThreads;
    const int beg = min(nb, (int)threadIdx.x * per), end = min(nb, beg + per);
    int s = 0;
    for (int i = beg; i < end; ++i) s += blk[i];
    int total;
    int ex = block_exclusive_scan(s, &total);
    for (int i = beg; i < end; ++i) {
        const int v = blk[i];
        blk[i] = ex;
        ex += v;
    }
    if (threadIdx.x == 0) blk[nb] = total;
}

__global__ __launch_bounds__(kThreads) void scan_apply_kernel(const int* __restrict__ in, long L, const int* __restrict__ blk,
                                                              int* __restrict__ out) {
    const long base = (long)blockIdx.x * kScanBlock + threadIdx.x * kScanItems;
    int v[kScanItems], s = 0;
#pragma unroll
    for (int k = 0; k < kScanItems; ++k) {
        v[k] = base + k < L ? in[base + k] : 0;
        s += v[k];
    }
    int total;
    int ex = block_exclusive_scan(s, &total) + blk[blockIdx.x];
#pragma unroll
    for (int k = 0; k < kScanItems; ++k)
        if (base + k < L) {
            out[base + k] = ex;
            ex += v[k];
        }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) out[L] = blk[gridDim.x];
}

// ---- validity + compaction ---------------------------------------------------------------------
__device__ __forceinline__ bool point_valid(float x, float y, float z) {
    if (!(isfinite(x) && isfinite(y) && isfinite(z))) return false;
    const double dx = x, dy = y, dz = z;
    return dx * dx + dy * dy + dz * dz > 1e-12;
}

__global__ __launch_bounds__(kThreads) void valid_flags_kernel(const float* __restrict__ p, long n, int* __restrict__ flag) {
    const long i = (long)blockIdx.x * kThreads + threadIdx.x;
    if (i < n) flag[i] = point_valid(p[i * 3], p[i * 3 + 1], p[i * 3 + 2]) ? 1 : 0;
}

__global__ __launch_bounds__(kThreads) void compact_kernel(const float* __restrict__ p, long n, const int* __restrict__ flag,
                                                           const int* __restrict__ pos, float* __restrict__ out,
                                                           int* __restrict__ out_idx) {
    const long i = (long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n || !flag[i]) return;
    const int j = pos[i];
    out[j * 3] = p[i * 3];
    out[j * 3 + 1] = p[i * 3 + 1];
    out[j * 3 + 2] = p[i * 3 + 2];
    out_idx[j] = (int)i;
}

// ---- hashed grid ---------------------------------------------------------------------------------
// cell coordinate of one axis; clamping keeps neighbours (<= 1 cell apart) within one cell of each other
__device__ __forceinline__ int cell_coord(double v, double inv_h) {
    const double q = fmin(fmax(floor(v * inv_h), (double)-kCellClamp), (double)kCellClamp);
    return (int)q;
}

__device__ __forceinline__ unsigned bucket_of(int cx, int cy, int cz, unsigned mask) {
    unsigned h = (unsigned)cx * 73856093u ^ (unsigned)cy * 19349663u ^ (unsigned)cz * 83492791u;
    h ^= h >> 16;   // murmur3 finaliser: the low bits that the mask keeps depend on every coordinate bit
    h *= 0x85ebca6bu;
    h ^= h >> 13;
    h *= 0xc2b2ae35u;
    h ^= h >> 16;
    return h & mask;
}

// neighbour k = 0..26 of a cell: offsets in the order 0, -1, +1 per axis (x fastest), so k = 0 is the cell itself
__device__ __forceinline__ int nb_off(int k) { return k == 0 ? 0 : (k == 1 ? -1 : 1); }

__global__ __launch_bounds__(kThreads) void grid_count_kernel(const float* __restrict__ p, int n, double inv_h, unsigned mask,
                                                              int* __restrict__ bucket, int* __restrict__ count) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const unsigned b = bucket_of(cell_coord(p[i * 3], inv_h), cell_coord(p[i * 3 + 1], inv_h), cell_coord(p[i * 3 + 2], inv_h), mask);
    bucket[i] = (int)b;
    atomicAdd(&count[b], 1);
}

__global__ __launch_bounds__(kThreads) void grid_scatter_kernel(int n, const int* __restrict__ bucket, const int* __restrict__ off,
                                                                int* __restrict__ cursor, int* __restrict__ order) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const int b = bucket[i];
    order[off[b] + atomicAdd(&cursor[b], 1)] = i;
}

// the scatter's order inside a bucket follows atomic arrival; the rank of an index among its bucket's indices
// puts every bucket in ascending point order, independent of that arrival order
__global__ __launch_bounds__(kThreads) void grid_sort_kernel(const float* __restrict__ p, int n, const int* __restrict__ bucket,
                                                             const int* __restrict__ off, const int* __restrict__ order,
                                                             float4* __restrict__ cell_pts) {
    const int q = blockIdx.x * kThreads + threadIdx.x;
    if (q >= n) return;
    const int i = order[q];
    const int b = bucket[i];
    const int beg = off[b], end = off[b + 1];
    int rank = 0;
    for (int k = beg; k < end; ++k) rank += order[k] < i;
    cell_pts[beg + rank] = make_float4(p[i * 3], p[i * 3 + 1], p[i * 3 + 2], __int_as_float(i));
}

// ---- normals -------------------------------------------------------------------------------------
// smallest-eigenvalue eigenvector of a symmetric 3x3 (cyclic Jacobi, float64, to convergence)
__device__ void smallest_eigvec3(double A[3][3], double n[3]) {
    double Q[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    for (int sweep = 0; sweep < 50; ++sweep) {
        const double off = A[0][1] * A[0][1] + A[0][2] * A[0][2] + A[1][2] * A[1][2];
        const double diag = A[0][0] * A[0][0] + A[1][1] * A[1][1] + A[2][2] * A[2][2];
        if (off == 0.0 || off <= 1e-40 * diag) break;
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int q = p + 1; q < 3; ++q) {
                if (A[p][q] == 0.0) continue;
                const double theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
                const double tn = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double cs = 1.0 / sqrt(tn * tn + 1.0), sn = tn * cs;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const double akp = A[k][p], akq = A[k][q];
                    A[k][p] = cs * akp - sn * akq;
                    A[k][q] = sn * akp + cs * akq;
                }
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const double apk = A[p][k], aqk = A[q][k];
                    A[p][k] = cs * apk - sn * aqk;
                    A[q][k] = sn * apk + cs * aqk;
                }
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const double qkp = Q[k][p], qkq = Q[k][q];
                    Q[k][p] = cs * qkp - sn * qkq;
                    Q[k][q] = sn * qkp + cs * qkq;
                }
            }
    }
    int best = 0;
    if (A[1][1] < A[best][best]) best = 1;
    if (A[2][2] < A[best][best]) best = 2;
    const double a = best == 0 ? Q[0][0] : (best == 1 ? Q[0][1] : Q[0][2]);
    const double b = best == 0 ? Q[1][0] : (best == 1 ? Q[1][1] : Q[1][2]);
    const double c = best == 0 ? Q[2][0] : (best == 1 ? Q[2][1] : Q[2][2]);
    const double s = 1.0 / sqrt(a * a + b * b + c * c);
    n[0] = a * s;
    n[1] = b * s;
    n[2] = c * s;
}

// one thread per grid position: the neighbours at d^2 < r2 over the 27 cells around the point (each bucket once,
// cells in the fixed nb_off order, points in index order inside a bucket) -> cumulants -> covariance -> normal.
// cell_nrm is indexed like cell_pts; normals_out / count_out (optional) by the original point index.
__global__ __launch_bounds__(kThreads) void normals_kernel(const float4* __restrict__ cell_pts, int n, const int* __restrict__ off,
                                                           unsigned mask, double inv_h, double r2, const int* __restrict__ orig,
                                                           double* __restrict__ cell_nrm, double* __restrict__ normals_out,
                                                           int* __restrict__ count_out) {
    const int q = blockIdx.x * kThreads + threadIdx.x;
    if (q >= n) return;
    const float4 c = cell_pts[q];
    const double px = c.x, py = c.y, pz = c.z;
    const int cx = cell_coord(px, inv_h), cy = cell_coord(py, inv_h), cz = cell_coord(pz, inv_h);
    int cnt = 0;
    double s0 = 0, s1 = 0, s2 = 0, s00 = 0, s01 = 0, s02 = 0, s11 = 0, s12 = 0, s22 = 0;
    for (int k = 0; k < 27; ++k) {
        const unsigned b = bucket_of(cx + nb_off(k % 3), cy + nb_off(k / 3 % 3), cz + nb_off(k / 9), mask);
        bool dup = false;
        for (int j = 0; j < k; ++j) dup |= bucket_of(cx + nb_off(j % 3), cy + nb_off(j / 3 % 3), cz + nb_off(j / 9), mask) == b;
        if (dup) continue;
        const int end = off[b + 1];
        for (int t = off[b]; t < end; ++t) {
            const float4 o = cell_pts[t];
            const double x = o.x, y = o.y, z = o.z;
            const double dx = x - px, dy = y - py, dz = z - pz;
            if (dx * dx + dy * dy + dz * dz < r2) {
                ++cnt;
                s0 += x;
                s1 += y;
                s2 += z;
                s00 += x * x;
                s01 += x * y;
                s02 += x * z;
                s11 += y * y;
                s12 += y * z;
                s22 += z * z;
            }
        }
    }
    double nv[3] = {0.0, 0.0, 1.0};
    if (cnt >= 3) {   // Open3D's ComputeCovariance: cumulants / n, then E[x x^T] - mean mean^T
        const double inv = 1.0 / cnt;
        const double m0 = s0 * inv, m1 = s1 * inv, m2 = s2 * inv;
        double A[3][3];
        A[0][0] = s00 * inv - m0 * m0;
        A[0][1] = A[1][0] = s01 * inv - m0 * m1;
        A[0][2] = A[2][0] = s02 * inv - m0 * m2;
        A[1][1] = s11 * inv - m1 * m1;
        A[1][2] = A[2][1] = s12 * inv - m1 * m2;
        A[2][2] = s22 * inv - m2 * m2;
        smallest_eigvec3(A, nv);
    }
    cell_nrm[q * 3] = nv[0];
    cell_nrm[q * 3 + 1] = nv[1];
    cell_nrm[q * 3 + 2] = nv[2];
    if (normals_out) {
        const int i = orig[__float_as_int(c.w)];
        normals_out[(long)i * 3] = nv[0];
        normals_out[(long)i * 3 + 1] = nv[1];
        normals_out[(long)i * 3 + 2] = nv[2];
        count_out[i] = cnt;
    }
}

// ---- one ICP iteration -----------------------------------------------------------------------------
// One thread per valid source point: y = T s (float64, from the original float32 s), nearest target point at
// d^2 < r2 (ties -> smaller index), then r = (y - t).n, J = [y x n ; n] -> 21 JtJ + 6 Jtr + d^2 + 1, reduced in a
// fixed order to one partial per workgroup (partial[blockIdx.x * kSlab + k]).  corr (optional): the correspondence's
// original target index at the source point's original index.
template <bool kSystem>
__global__ __launch_bounds__(kThreads) void icp_iter_kernel(const float* __restrict__ src, int n_src, const float4* __restrict__ cell_pts,
                                                            const double* __restrict__ cell_nrm, const int* __restrict__ off,
                                                            unsigned mask, double inv_h, double h, double r2, Mat34 T,
                                                            double* __restrict__ partial, const int* __restrict__ src_orig,
                                                            const int* __restrict__ tgt_orig, int* __restrict__ corr) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    double acc[kSums];
#pragma unroll
    for (int k = 0; k < kSums; ++k) acc[k] = 0.0;
    if (i < n_src) {
        const double sx = src[i * 3], sy = src[i * 3 + 1], sz = src[i * 3 + 2];
        const double y0 = T.m[0] * sx + T.m[1] * sy + T.m[2] * sz + T.m[3];
        const double y1 = T.m[4] * sx + T.m[5] * sy + T.m[6] * sz + T.m[7];
        const double y2 = T.m[8] * sx + T.m[9] * sy + T.m[10] * sz + T.m[11];
        const int cx = cell_coord(y0, inv_h), cy = cell_coord(y1, inv_h), cz = cell_coord(y2, inv_h);
        const double pad = h * 1e-6;   // > any cell misassignment by rounding (|coordinate| <= kCellClamp * h)
        double best = r2;
        int best_idx = 0x7fffffff, best_pos = -1;
        for (int k = 0; k < 27; ++k) {
            const int ax = cx + nb_off(k % 3), ay = cy + nb_off(k / 3 % 3), az = cz + nb_off(k / 9);
            if (abs(ax) < kCellClamp && abs(ay) < kCellClamp && abs(az) < kCellClamp) {
                // prune: lower bound of the distance from y to the (padded) cell box
                const double gx = fmax(fmax(ax * h - pad - y0, y0 - (ax + 1) * h - pad), 0.0);
                const double gy = fmax(fmax(ay * h - pad - y1, y1 - (ay + 1) * h - pad), 0.0);
                const double gz = fmax(fmax(az * h - pad - y2, y2 - (az + 1) * h - pad), 0.0);
                if (gx * gx + gy * gy + gz * gz > best) continue;
            }
            const unsigned b = bucket_of(ax, ay, az, mask);
            const int end = off[b + 1];
            for (int t = off[b]; t < end; ++t) {
                const float4 o = cell_pts[t];
                const double dx = y0 - (double)o.x, dy = y1 - (double)o.y, dz = y2 - (double)o.z;
                const double d2 = dx * dx + dy * dy + dz * dz;
                const int idx = __float_as_int(o.w);
                if (d2 < best || (best_pos >= 0 && d2 == best && idx < best_idx)) {
                    best = d2;
                    best_idx = idx;
                    best_pos = t;
                }
            }
        }
        if (corr) corr[src_orig[i]] = best_pos >= 0 ? tgt_orig[best_idx] : -1;
        if (kSystem && best_pos >= 0) {
            const float4 o = cell_pts[best_pos];
            const double n0 = cell_nrm[best_pos * 3], n1 = cell_nrm[best_pos * 3 + 1], n2 = cell_nrm[best_pos * 3 + 2];
            const double r = (y0 - (double)o.x) * n0 + (y1 - (double)o.y) * n1 + (y2 - (double)o.z) * n2;
            const double J[6] = {y1 * n2 - y2 * n1, y2 * n0 - y0 * n2, y0 * n1 - y1 * n0, n0, n1, n2};
            int k = 0;
#pragma unroll
            for (int a = 0; a < 6; ++a)
#pragma unroll
                for (int c = a; c < 6; ++c) acc[k++] = J[a] * J[c];
#pragma unroll
            for (int a = 0; a < 6; ++a) acc[21 + a] = J[a] * r;
            acc[27] = best;
            acc[28] = 1.0;
        }
    }
    if (!kSystem) return;
    __shared__ double wpart[kThreads / 64][kSums];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < kSums; ++k) {
        const double v = wave_sum(acc[k]);
        if (lane == 0) wpart[wave][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < kSums) {
        double s = 0.0;
#pragma unroll
        for (int w = 0; w < kThreads / 64; ++w) s += wpart[w][threadIdx.x];
        partial[(long)blockIdx.x * kSlab + threadIdx.x] = s;
    }
}

// one workgroup: sums[k] = sum over the nb partials of value k, in a fixed order.  Thread t adds value t % 32 of the
// partials t / 32, t / 32 + 8, ... (each group of 32 threads reads whole slab rows), then the 8 group sums in order.
__global__ __launch_bounds__(kThreads) void icp_sum_kernel(const double* __restrict__ partial, int nb, double* __restrict__ sums) {
    constexpr int kGroups = kThreads / kSlab;
    __shared__ double gpart[kGroups][kSlab];
    const int k = threadIdx.x % kSlab, g = threadIdx.x / kSlab;
    double s = 0.0;
    for (int b = g; b < nb; b += kGroups) s += partial[(long)b * kSlab + k];
    gpart[g][k] = s;
    __syncthreads();
    if (threadIdx.x < kSums) {
        double t = 0.0;
#pragma unroll
        for (int j = 0; j < kGroups; ++j) t += gpart[j][threadIdx.x];
        sums[threadIdx.x] = t;
    }
}

// ---- host side -----------------------------------------------------------------------------------
struct Layout {
    size_t src_pts, src_idx, tgt_pts, tgt_idx, tgt_bucket, order, cell_pts, cell_nrm, cnt, off, cursor, flag, pos, blk,
        partial, sums, total;
    unsigned table;   // buckets (power of two)
    int scan_blocks;
};

Layout layout(long n_src, long n_tgt) {
    Layout L;
    unsigned tb = 1024;
    while ((long)tb < 2 * n_tgt) tb <<= 1;
    L.table = tb;
    const long nmax = std::max({n_src, n_tgt, (long)tb});
    L.scan_blocks = (int)cdiv(nmax, kScanBlock);
    size_t o = 0;
    auto take = [&](size_t bytes) {
        const size_t at = o;
        o = align_up(o + std::max<size_t>(bytes, 1), 256);
        return at;
    };
    L.src_pts = take((size_t)n_src * 12);
    L.src_idx = take((size_t)n_src * 4);
    L.tgt_pts = take((size_t)n_tgt * 12);
    L.tgt_idx = take((size_t)n_tgt * 4);
    L.tgt_bucket = take((size_t)n_tgt * 4);
    L.order = take((size_t)n_tgt * 4);
    L.cell_pts = take((size_t)n_tgt * 16);
    L.cell_nrm = take((size_t)n_tgt * 24);
    L.cnt = take((size_t)tb * 4);
    L.off = take(((size_t)tb + 1) * 4);
    L.cursor = take((size_t)tb * 4);
    L.flag = take((size_t)std::max(n_src, n_tgt) * 4);
    L.pos = take(((size_t)std::max(n_src, n_tgt) + 1) * 4);
    L.blk = take(((size_t)L.scan_blocks + 1) * 4);
    L.partial = take((size_t)cdiv(std::max(n_src, 1L), kThreads) * kSlab * 8);
    L.sums = take(kSlab * 8);
    L.total = o;
    return L;
}

template <class P>
P* at(void* ws, size_t offset) {
    return reinterpret_cast<P*>(static_cast<char*>(ws) + offset);
}

unsigned grid1(long n) { return (unsigned)cdiv(std::max(n, 1L), kThreads); }

int exclusive_scan(const int* in, long n, int* blk, int* out, hipStream_t st) {
    const int nb = (int)cdiv(std::max(n, 1L), kScanBlock);
    hipLaunchKernelGGL(scan_block_sums_kernel, dim3(nb), dim3(kThreads), 0, st, in, n, blk);
    hipLaunchKernelGGL(scan_top_kernel, dim3(1), dim3(kThreads), 0, st, blk, nb);
    hipLaunchKernelGGL(scan_apply_kernel, dim3(nb), dim3(kThreads), 0, st, in, n, blk, out);
    SKIMI_LAUNCH_CHECK();
    return SKIMI_OK;
}

// valid points of p [n, 3] -> out [nv, 3] in original order, out_idx = their original indices; *nv read back
int compact(const float* p, long n, const Layout& L, void* ws, float* out, int* out_idx, int* nv, hipStream_t st) {
    *nv = 0;
    if (n == 0) return SKIMI_OK;
    int* flag = at<int>(ws, L.flag);
    int* pos = at<int>(ws, L.pos);
    hipLaunchKernelGGL(valid_flags_kernel, dim3(grid1(n)), dim3(kThreads), 0, st, p, n, flag);
    int rc = exclusive_scan(flag, n, at<int>(ws, L.blk), pos, st);
    if (rc != SKIMI_OK) return rc;
    hipLaunchKernelGGL(compact_kernel, dim3(grid1(n)), dim3(kThreads), 0, st, p, n, flag, pos, out, out_idx);
    SKIMI_LAUNCH_CHECK();
    SKIMI_HIP(hipMemcpyAsync(nv, pos + n, sizeof(int), hipMemcpyDeviceToHost, st));
    SKIMI_HIP(hipStreamSynchronize(st));
    return SKIMI_OK;
}

// the target's grid: cell_pts sorted by bucket, then by index; off[b] .. off[b + 1] = bucket b
int build_grid(int nv, double h, const Layout& L, void* ws, hipStream_t st) {
    const unsigned mask = L.table - 1;
    int* cnt = at<int>(ws, L.cnt);
    int* off = at<int>(ws, L.off);
    int* cursor = at<int>(ws, L.cursor);
    int* bucket = at<int>(ws, L.tgt_bucket);
    const float* pts = at<float>(ws, L.tgt_pts);
    SKIMI_HIP(hipMemsetAsync(cnt, 0, (size_t)L.table * 4, st));
    SKIMI_HIP(hipMemsetAsync(cursor, 0, (size_t)L.table * 4, st));
    hipLaunchKernelGGL(grid_count_kernel, dim3(grid1(nv)), dim3(kThreads), 0, st, pts, nv, 1.0 / h, mask, bucket, cnt);
    int rc = exclusive_scan(cnt, L.table, at<int>(ws, L.blk), off, st);
    if (rc != SKIMI_OK) return rc;
    hipLaunchKernelGGL(grid_scatter_kernel, dim3(grid1(nv)), dim3(kThreads), 0, st, nv, bucket, off, cursor, at<int>(ws, L.order));
    hipLaunchKernelGGL(grid_sort_kernel, dim3(grid1(nv)), dim3(kThreads), 0, st, pts, nv, bucket, off, at<int>(ws, L.order),
                       at<float4>(ws, L.cell_pts));
    SKIMI_LAUNCH_CHECK();
    return SKIMI_OK;
}

int launch_normals(int nv, double h, double radius, const Layout& L, void* ws, double* normals_out, int* count_out, hipStream_t st) {
    hipLaunchKernelGGL(normals_kernel, dim3(grid1(nv)), dim3(kThreads), 0, st, at<float4>(ws, L.cell_pts), nv, at<int>(ws, L.off),
                       L.table - 1, 1.0 / h, radius * radius, at<int>(ws, L.tgt_idx), at<double>(ws, L.cell_nrm), normals_out,
                       count_out);
    SKIMI_LAUNCH_CHECK();
    return SKIMI_OK;
}

Mat34 to_mat34(const double* T) {
    Mat34 m;
    for (int k = 0; k < 12; ++k) m.m[k] = T[k];
    return m;
}

// JtJ x = -Jtr by LDLT with diagonal pivoting (largest remaining diagonal first, as Eigen's LDLT); a pivot of
// magnitude <= DBL_MIN contributes 0 to x (Eigen's solve).  false if x is not finite.
bool solve6_ldlt(const double* sums, double x[6]) {
    double A[6][6], b[6];
    int k = 0;
    for (int a = 0; a < 6; ++a)
        for (int c = a; c < 6; ++c) A[a][c] = A[c][a] = sums[k++];
    for (int a = 0; a < 6; ++a) b[a] = -sums[21 + a];
    int perm[6] = {0, 1, 2, 3, 4, 5};
    double D[6];
    for (int j = 0; j < 6; ++j) {
        int piv = j;
        for (int i = j + 1; i < 6; ++i)
            if (fabs(A[i][i]) > fabs(A[piv][piv])) piv = i;
        if (piv != j) {
            for (int c = 0; c < 6; ++c) std::swap(A[j][c], A[piv][c]);
            for (int r = 0; r < 6; ++r) std::swap(A[r][j], A[r][piv]);
            std::swap(perm[j], perm[piv]);
        }
        D[j] = A[j][j];
        for (int i = j + 1; i < 6; ++i) A[i][j] = fabs(D[j]) > 2.2250738585072014e-308 ? A[i][j] / D[j] : 0.0;   // L[i][j]
        for (int i = j + 1; i < 6; ++i)
            for (int c = j + 1; c <= i; ++c) {
                A[i][c] -= A[i][j] * D[j] * A[c][j];
                A[c][i] = A[i][c];
            }
    }
    double y[6];
    for (int i = 0; i < 6; ++i) y[i] = b[perm[i]];
    for (int i = 0; i < 6; ++i)
        for (int c = 0; c < i; ++c) y[i] -= A[i][c] * y[c];
    for (int i = 0; i < 6; ++i) y[i] = fabs(D[i]) > 2.2250738585072014e-308 ? y[i] / D[i] : 0.0;
    for (int i = 5; i >= 0; --i)
        for (int c = i + 1; c < 6; ++c) y[i] -= A[c][i] * y[c];
    for (int i = 0; i < 6; ++i) x[perm[i]] = y[i];
    for (int i = 0; i < 6; ++i)
        if (!std::isfinite(x[i])) return false;
    return true;
}

// x -> 4x4: R = Rz(x2) Ry(x1) Rx(x0), translation x3..5 (Open3D's TransformVector6dToMatrix4d)
void euler_to_mat(const double x[6], double U[16]) {
    const double ca = cos(x[0]), sa = sin(x[0]), cb = cos(x[1]), sb = sin(x[1]), cg = cos(x[2]), sg = sin(x[2]);
    const double Rx[3][3] = {{1, 0, 0}, {0, ca, -sa}, {0, sa, ca}};
    const double Ry[3][3] = {{cb, 0, sb}, {0, 1, 0}, {-sb, 0, cb}};
    const double Rz[3][3] = {{cg, -sg, 0}, {sg, cg, 0}, {0, 0, 1}};
    double Ryx[3][3];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) Ryx[r][c] = Ry[r][0] * Rx[0][c] + Ry[r][1] * Rx[1][c] + Ry[r][2] * Rx[2][c];
    for (int k = 0; k < 16; ++k) U[k] = (k % 5 == 0) ? 1.0 : 0.0;
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) U[r * 4 + c] = Rz[r][0] * Ryx[0][c] + Rz[r][1] * Ryx[1][c] + Rz[r][2] * Ryx[2][c];
        U[r * 4 + 3] = x[3 + r];
    }
}

void matmul4(const double* A, const double* B, double* C) {
    double t[16];
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) t[r * 4 + c] = A[r * 4] * B[c] + A[r * 4 + 1] * B[4 + c] + A[r * 4 + 2] * B[8 + c] + A[r * 4 + 3] * B[12 + c];
    for (int k = 0; k < 16; ++k) C[k] = t[k];
}

}  // namespace
}  // namespace skimi

using namespace skimi;

extern "C" {

size_t skimi_icp_workspace_bytes(int64_t n_src, int64_t n_tgt) {
    if (n_src < 0 || n_tgt < 0) return 0;
    return layout((long)n_src, (long)n_tgt).total;
}

int skimi_estimate_normals(const float* points, int64_t n, double radius, double* normals_out, int32_t* neighbour_count_out,
                           void* ws, size_t ws_bytes, void* stream) {
    SKIMI_CHECK_ARG(points && normals_out && neighbour_count_out && ws && n >= 0 && n < (1L << 30) && radius > 0,
                    "skimi_estimate_normals: bad arguments");
    const Layout L = layout(0, (long)n);
    SKIMI_CHECK_ARG(ws_bytes >= L.total, "skimi_estimate_normals: workspace of %zu bytes < skimi_icp_workspace_bytes(0, n) = %zu",
                    ws_bytes, L.total);
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) return SKIMI_OK;
    SKIMI_HIP(hipMemsetAsync(normals_out, 0, (size_t)n * 24, st));
    SKIMI_HIP(hipMemsetAsync(neighbour_count_out, 0, (size_t)n * 4, st));
    int nv = 0;
    int rc = compact(points, (long)n, L, ws, at<float>(ws, L.tgt_pts), at<int>(ws, L.tgt_idx), &nv, st);
    if (rc != SKIMI_OK || nv == 0) return rc;
    const double h = radius * kCellPad;
    rc = build_grid(nv, h, L, ws, st);
    if (rc != SKIMI_OK) return rc;
    return launch_normals(nv, h, radius, L, ws, normals_out, neighbour_count_out, st);
}

int skimi_icp_correspondences(const float* src, int64_t n_src, const float* tgt, int64_t n_tgt, const double* T4x4,
                              double max_dist, int32_t* tgt_index_out, void* ws, size_t ws_bytes, void* stream) {
    SKIMI_CHECK_ARG(src && tgt && T4x4 && tgt_index_out && ws && n_src >= 0 && n_tgt >= 0 && n_src < (1L << 30) &&
                        n_tgt < (1L << 30) && max_dist > 0,
                    "skimi_icp_correspondences: bad arguments");
    const Layout L = layout((long)n_src, (long)n_tgt);
    SKIMI_CHECK_ARG(ws_bytes >= L.total, "skimi_icp_correspondences: workspace of %zu bytes < skimi_icp_workspace_bytes = %zu",
                    ws_bytes, L.total);
    hipStream_t st = (hipStream_t)stream;
    if (n_src == 0) return SKIMI_OK;
    SKIMI_HIP(hipMemsetAsync(tgt_index_out, 0xff, (size_t)n_src * 4, st));   // -1: no correspondence
    int ns = 0, nt = 0;
    int rc = compact(src, (long)n_src, L, ws, at<float>(ws, L.src_pts), at<int>(ws, L.src_idx), &ns, st);
    if (rc == SKIMI_OK) rc = compact(tgt, (long)n_tgt, L, ws, at<float>(ws, L.tgt_pts), at<int>(ws, L.tgt_idx), &nt, st);
    if (rc != SKIMI_OK || ns == 0 || nt == 0) return rc;
    const double h = max_dist * kCellPad;
    rc = build_grid(nt, h, L, ws, st);
    if (rc != SKIMI_OK) return rc;
    hipLaunchKernelGGL(icp_iter_kernel<false>, dim3(grid1(ns)), dim3(kThreads), 0, st, at<float>(ws, L.src_pts), ns,
                       at<float4>(ws, L.cell_pts), (const double*)nullptr, at<int>(ws, L.off), L.table - 1, 1.0 / h, h,
                       max_dist * max_dist, to_mat34(T4x4), (double*)nullptr, at<int>(ws, L.src_idx), at<int>(ws, L.tgt_idx),
                       tgt_index_out);
    SKIMI_LAUNCH_CHECK();
    return SKIMI_OK;
}

int skimi_icp_point_to_plane(const float* src, int64_t n_src, const float* tgt, int64_t n_tgt, double max_corr_dist,
                             double normal_radius, int32_t max_iteration, double rel_fitness, double rel_rmse,
                             const double* init4x4, double* T_out, double* fitness_out, double* rmse_out,
                             int32_t* iterations_out, void* ws, size_t ws_bytes, void* stream) {
    SKIMI_CHECK_ARG(src && tgt && T_out && fitness_out && rmse_out && iterations_out && ws && n_src >= 0 && n_tgt >= 0 &&
                        n_src < (1L << 30) && n_tgt < (1L << 30) && max_corr_dist > 0 && normal_radius > 0 && max_iteration >= 0,
                    "skimi_icp_point_to_plane: bad arguments");
    const Layout L = layout((long)n_src, (long)n_tgt);
    SKIMI_CHECK_ARG(ws_bytes >= L.total, "skimi_icp_point_to_plane: workspace of %zu bytes < skimi_icp_workspace_bytes = %zu",
                    ws_bytes, L.total);
    hipStream_t st = (hipStream_t)stream;
    for (int k = 0; k < 16; ++k) T_out[k] = (k % 5 == 0) ? 1.0 : 0.0;
    *fitness_out = 0.0;
    *rmse_out = 0.0;
    *iterations_out = 0;
    int ns = 0, nt = 0;
    int rc = compact(src, (long)n_src, L, ws, at<float>(ws, L.src_pts), at<int>(ws, L.src_idx), &ns, st);
    if (rc == SKIMI_OK) rc = compact(tgt, (long)n_tgt, L, ws, at<float>(ws, L.tgt_pts), at<int>(ws, L.tgt_idx), &nt, st);
    if (rc != SKIMI_OK) return rc;
    if (ns < kMinPoints || nt < kMinPoints) return SKIMI_OK;   // eye(4): multi_view_process.py:471-474
    const double h = std::max(max_corr_dist, normal_radius) * kCellPad;
    rc = build_grid(nt, h, L, ws, st);
    if (rc == SKIMI_OK) rc = launch_normals(nt, h, normal_radius, L, ws, nullptr, nullptr, st);
    if (rc != SKIMI_OK) return rc;

    double T[16];
    for (int k = 0; k < 16; ++k) T[k] = init4x4 ? init4x4[k] : ((k % 5 == 0) ? 1.0 : 0.0);
    const int nb = (int)grid1(ns);
    double* partial = at<double>(ws, L.partial);
    double* dsums = at<double>(ws, L.sums);
    double sums[kSlab];
    // evaluate(T): correspondences of T s, their 6x6 system, fitness and RMSE
    auto evaluate = [&](double* fit, double* rmse) -> int {
        hipLaunchKernelGGL(icp_iter_kernel<true>, dim3(nb), dim3(kThreads), 0, st, at<float>(ws, L.src_pts), ns,
                           at<float4>(ws, L.cell_pts), at<double>(ws, L.cell_nrm), at<int>(ws, L.off), L.table - 1, 1.0 / h, h,
                           max_corr_dist * max_corr_dist, to_mat34(T), partial, (const int*)nullptr, (const int*)nullptr,
                           (int*)nullptr);
        hipLaunchKernelGGL(icp_sum_kernel, dim3(1), dim3(kThreads), 0, st, partial, nb, dsums);
        SKIMI_LAUNCH_CHECK();
        SKIMI_HIP(hipMemcpyAsync(sums, dsums, kSums * sizeof(double), hipMemcpyDeviceToHost, st));
        SKIMI_HIP(hipStreamSynchronize(st));
        const double ncorr = sums[28];
        *fit = ncorr / ns;
        *rmse = ncorr > 0 ? sqrt(sums[27] / ncorr) : 0.0;
        return SKIMI_OK;
    };
    double fit = 0, rmse = 0;
    rc = evaluate(&fit, &rmse);
    if (rc != SKIMI_OK) return rc;
    int it = 0;
    for (; it < max_iteration;) {
        double U[16];
        double x[6];
        if (sums[28] > 0 && solve6_ldlt(sums, x))
            euler_to_mat(x, U);
        else
            for (int k = 0; k < 16; ++k) U[k] = (k % 5 == 0) ? 1.0 : 0.0;
        matmul4(U, T, T);
        ++it;
        const double fit0 = fit, rmse0 = rmse;
        rc = evaluate(&fit, &rmse);
        if (rc != SKIMI_OK) return rc;
        if (fabs(fit0 - fit) < rel_fitness && fabs(rmse0 - rmse) < rel_rmse) break;
    }
    for (int k = 0; k < 16; ++k) T_out[k] = T[k];
    *fitness_out = fit;
    *rmse_out = rmse;
    *iterations_out = it;
    return SKIMI_OK;
}

}  // extern "C"
