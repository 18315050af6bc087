// Geometry post-processing of the VGGT outputs, on device so the dense maps never leave HBM:
//   pose encoding -> extrinsics / intrinsics   (vggt/vggt/utils/pose_enc.py:62-124, rotation.py:14-44)
//   depth map -> world points                  (vggt/vggt/utils/geometry.py:15-117)
//   DLT triangulation of 2D joints over V views (vggt/triangulate.py:13-34, generalised from 2 to V
//                                               views: two rows of A per view)
#include <algorithm>

#include "common.h"

namespace skimi {

// [R, 9] = (T[3], quat xyzw[4], fov_h, fov_w) -> E [R,3,4] = [R(q) | T], K [R,3,3]
__global__ void pose_to_cameras_kernel(const float* __restrict__ pose, float* __restrict__ E, float* __restrict__ K,
                                       long rows, float H, float W) {
    const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    const float* p = pose + r * 9;
    const float i = p[3], j = p[4], k = p[5], w = p[6];
    const float two_s = 2.0f / (i * i + j * j + k * k + w * w);   // rotation.py:27
    float* e = E + r * 12;
    e[0] = 1 - two_s * (j * j + k * k); e[1] = two_s * (i * j - k * w); e[2] = two_s * (i * k + j * w); e[3] = p[0];
    e[4] = two_s * (i * j + k * w); e[5] = 1 - two_s * (i * i + k * k); e[6] = two_s * (j * k - i * w); e[7] = p[1];
    e[8] = two_s * (i * k - j * w); e[9] = two_s * (j * k + i * w); e[10] = 1 - two_s * (i * i + j * j); e[11] = p[2];
    if (K) {
        float* q = K + r * 9;
        const float fy = (H / 2.0f) / tanf(p[7] / 2.0f);   // pose_enc.py:112-113
        const float fx = (W / 2.0f) / tanf(p[8] / 2.0f);
        q[0] = fx; q[1] = 0; q[2] = W / 2; q[3] = 0; q[4] = fy; q[5] = H / 2; q[6] = 0; q[7] = 0; q[8] = 1;
    }
}

// world = R^T (cam - t), cam = ((u-cx) d / fx, (v-cy) d / fy, d)   (geometry.py:47-117)
__global__ __launch_bounds__(256) void unproject_kernel(const float* __restrict__ depth, const float* __restrict__ E,
                                                        const float* __restrict__ K, float* __restrict__ out, int F, int H,
                                                        int W) {
    const long total = (long)F * H * W;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int u = (int)(i % W);
        const int v = (int)((i / W) % H);
        const long f = i / ((long)W * H);
        const float* e = E + f * 12;
        const float* k = K + f * 9;
        const float d = depth[i];
        const float x = ((float)u - k[2]) * d / k[0];
        const float y = ((float)v - k[5]) * d / k[4];
        const float z = d;
        // cam-to-world = [R^T | -R^T t] (closed_form_inverse_se3); points . R_c2w^T + t_c2w
        const float tx = -(e[0] * e[3] + e[4] * e[7] + e[8] * e[11]);
        const float ty = -(e[1] * e[3] + e[5] * e[7] + e[9] * e[11]);
        const float tz = -(e[2] * e[3] + e[6] * e[7] + e[10] * e[11]);
        out[i * 3 + 0] = x * e[0] + y * e[4] + z * e[8] + tx;
        out[i * 3 + 1] = x * e[1] + y * e[5] + z * e[9] + ty;
        out[i * 3 + 2] = x * e[2] + y * e[6] + z * e[10] + tz;
    }
}

// One (time step, joint): A = rows {u P[2] - P[0], v P[1]...} over V views, the
// solution is the right-singular vector of A for the smallest singular value = eigenvector of
// A^T A (4x4, symmetric) for the smallest eigenvalue; cyclic Jacobi in double precision.
// The pieces are shared by the plain, the triage and the robust kernel: camera_P forms P = K [R | t], dlt_add_view adds
// one view's two rows onto M = A^T A, dlt_solve is the eigen-solve -> (X / X[3])[:3] in float64.  Every 4 x 4 array is
// indexed by constants once the loops are unrolled, so none of them goes to scratch memory.
__device__ __forceinline__ void camera_P(const float* __restrict__ K, const float* __restrict__ R,
                                         const float* __restrict__ tt, double* __restrict__ P) {
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {   // P = K [R | t]  (triangulate.py:13-16)
            double s = 0;
#pragma unroll
            for (int c = 0; c < 3; ++c) s += (double)K[a * 3 + c] * (b < 3 ? (double)R[c * 3 + b] : (double)tt[c]);
            P[a * 4 + b] = s;
        }
}

// P: 12 doubles, row-major 3 x 4.  kScaled: both rows times s (the robust refit's confidence weight)
template <bool kScaled>
__device__ __forceinline__ void dlt_add_view(double (&M)[4][4], const double* P, double u, double w, double s) {
    double r0[4], r1[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        r0[b] = u * P[8 + b] - P[b];
        r1[b] = w * P[8 + b] - P[4 + b];
        if (kScaled) {
            r0[b] *= s;
            r1[b] *= s;
        }
    }
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) M[a][b] += r0[a] * r0[b] + r1[a] * r1[b];
}

__device__ __forceinline__ void dlt_solve(double (&M)[4][4], double (&X)[3]) {
    double Q[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
#pragma nounroll
    for (int sweep = 0; sweep < 30; ++sweep) {
        double off = 0;
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = a + 1; b < 4; ++b) off += M[a][b] * M[a][b];
        double diag = 0;
#pragma unroll
        for (int a = 0; a < 4; ++a) diag += M[a][a] * M[a][a];
        if (off <= 1e-40 * diag || off == 0.0) break;
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int q = p + 1; q < 4; ++q) {
                if (M[p][q] == 0.0) continue;
                const double theta = (M[q][q] - M[p][p]) / (2.0 * M[p][q]);
                const double tn = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double cs = 1.0 / sqrt(tn * tn + 1.0), sn = tn * cs;
#pragma unroll
                for (int k = 0; k < 4; ++k) {   // rotate columns p, q
                    const double mkp = M[k][p], mkq = M[k][q];
                    M[k][p] = cs * mkp - sn * mkq;
                    M[k][q] = sn * mkp + cs * mkq;
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {   // rotate rows p, q
                    const double mpk = M[p][k], mqk = M[q][k];
                    M[p][k] = cs * mpk - sn * mqk;
                    M[q][k] = sn * mpk + cs * mqk;
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const double qkp = Q[k][p], qkq = Q[k][q];
                    Q[k][p] = cs * qkp - sn * qkq;
                    Q[k][q] = sn * qkp + cs * qkq;
                }
            }
    }
    // the column of the smallest diagonal entry (the first of equals), picked by selects: no runtime index
    double lam = M[0][0], q0 = Q[0][0], q1 = Q[1][0], q2 = Q[2][0], wv = Q[3][0];
#pragma unroll
    for (int a = 1; a < 4; ++a)
        if (M[a][a] < lam) {
            lam = M[a][a];
            q0 = Q[0][a];
            q1 = Q[1][a];
            q2 = Q[2][a];
            wv = Q[3][a];
        }
    X[0] = q0 / wv;   // (X / X[3])[:3]  (triangulate.py:33-34)
    X[1] = q1 / wv;
    X[2] = q2 / wv;
}

// dlt_point is the solve over all V views for joint j of step t, shared by the plain and the triage kernel -> X rounded
// to float32.
__device__ __forceinline__ void dlt_point(const float* __restrict__ Kc, const float* __restrict__ Rc,
                                          const float* __restrict__ tc, const float* __restrict__ kp, long t, int j, int V,
                                          int J, float* __restrict__ o) {
    double M[4][4] = {{0}};
    for (int v = 0; v < V; ++v) {
        double P[12];
        camera_P(Kc + (t * V + v) * 9, Rc + (t * V + v) * 9, tc + (t * V + v) * 3, P);
        const double u = kp[((t * V + v) * J + j) * 2], w = kp[((t * V + v) * J + j) * 2 + 1];
        dlt_add_view<false>(M, P, u, w, 1.0);
    }
    double X[3];
    dlt_solve(M, X);
    o[0] = (float)X[0];
    o[1] = (float)X[1];
    o[2] = (float)X[2];
}

__global__ void triangulate_dlt_kernel(const float* __restrict__ Kc, const float* __restrict__ Rc,
                                       const float* __restrict__ tc, const float* __restrict__ kp, float* __restrict__ X,
                                       long T, int V, int J) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= T * J) return;
    const long t = idx / J;
    const int j = (int)(idx - t * J);
    dlt_point(Kc, Rc, tc, kp, t, j, V, J, X + idx * 3);
}

// Triangulation with a verdict (reproject_and_visualize, vggt/reproject.py:108-144, :334-341; post_triage_single,
// triangulation/postprocess.py:38-43, :102-121, from two views to V; rules: DESIGN §2 "Triage").  One workgroup per time
// step, thread j < J owns joint j: the DLT above, then the stored float32 X through every view's own K (R X + t) in
// float64.  After a barrier thread v < V reduces view v's errors over the joints and thread V the step's report, NaN-aware
// as nanmean / nanmedian / nanmax, every sum in joint order.
constexpr int kTriageMaxJ = 32, kTriageMaxV = 8;

// NaN-aware statistics of n <= 32 values: rmse, mean, median, max of the non-NaN ones (all NaN when there is none)
__device__ inline void nan_stats(const double* x, int n, double* rmse, double* mean, double* median, double* mx) {
    double s[kTriageMaxJ];
    int m = 0;
    double sum = 0, sq = 0, big = -INFINITY;
    for (int i = 0; i < n; ++i) {
        const double v = x[i];
        if (v != v) continue;
        sum += v;
        sq += v * v;
        big = v > big ? v : big;
        int k = m++;   // insertion sort: n is tiny
        while (k > 0 && s[k - 1] > v) {
            s[k] = s[k - 1];
            --k;
        }
        s[k] = v;
    }
    const double nan = __longlong_as_double(0x7FF8000000000000LL);
    if (rmse) *rmse = m ? sqrt(sq / m) : nan;
    if (mean) *mean = m ? sum / m : nan;
    if (median) *median = m ? ((m & 1) ? s[m / 2] : (s[m / 2 - 1] + s[m / 2]) / 2.0) : nan;
    if (mx) *mx = m ? big : nan;
}

__global__ __launch_bounds__(64) void triangulate_triage_kernel(
    const float* __restrict__ Kc, const float* __restrict__ Rc, const float* __restrict__ tc, const float* __restrict__ kp,
    const float* __restrict__ conf, double conf_thr, double err_thresh, int V, int J, float* __restrict__ X,
    float* __restrict__ X_clean, double* __restrict__ err, double* __restrict__ depth, unsigned char* __restrict__ keep,
    double* __restrict__ view_stats, double* __restrict__ report) {
    __shared__ double s_err[kTriageMaxV][kTriageMaxJ];
    __shared__ double s_em[kTriageMaxJ];
    __shared__ int s_pos[kTriageMaxJ], s_keep[kTriageMaxJ];
    const long t = blockIdx.x;
    const int j = threadIdx.x;
    if (j < J) {
        float x[3];
        dlt_point(Kc, Rc, tc, kp, t, j, V, J, x);
        bool pos = true, seen = true;
        double em = 0;
        for (int v = 0; v < V; ++v) {
            const float* K = Kc + (t * V + v) * 9;
            const float* R = Rc + (t * V + v) * 9;
            const float* tt = tc + (t * V + v) * 3;
            double c[3], p[3];
            for (int a = 0; a < 3; ++a) {
                double s = 0;
                for (int b = 0; b < 3; ++b) s += (double)R[a * 3 + b] * (double)x[b];
                c[a] = s + (double)tt[a];
            }
            for (int a = 0; a < 3; ++a) {
                double s = 0;
                for (int b = 0; b < 3; ++b) s += (double)K[a * 3 + b] * c[b];
                p[a] = s;
            }
            const long o = (t * V + v) * J + j;
            const double du = p[0] / p[2] - (double)kp[o * 2], dv = p[1] / p[2] - (double)kp[o * 2 + 1];
            const double e = sqrt(du * du + dv * dv);
            depth[o] = p[2];
            err[o] = e;
            s_err[v][j] = e;
            em += e;
            pos = pos && p[2] > 0;
            if (conf) seen = seen && (double)conf[o] >= conf_thr;
        }
        em /= (double)V;
        const bool k = pos && isfinite(em) && em <= err_thresh && seen;
        const float nanf_ = __uint_as_float(0x7FC00000u);
        for (int a = 0; a < 3; ++a) {
            X[(t * J + j) * 3 + a] = x[a];
            X_clean[(t * J + j) * 3 + a] = k ? x[a] : nanf_;
        }
        keep[t * J + j] = k ? 1 : 0;
        s_em[j] = em;
        s_pos[j] = pos;
        s_keep[j] = k;
    }
    __syncthreads();
    if (j < V) {
        double* o = view_stats + (t * V + j) * 4;
        nan_stats(s_err[j], J, o, o + 1, o + 2, o + 3);
    } else if (j == V) {
        double* o = report + t * 5;
        nan_stats(s_em, J, o, nullptr, o + 1, nullptr);
        int np = 0, nk = 0;
        for (int i = 0; i < J; ++i) {
            np += s_pos[i];
            nk += s_keep[i];
        }
        o[2] = (double)np / J;
        o[3] = (double)nk / J;
        o[4] = (double)nk;
    }
}


// Outlier-robust triangulation (rules: DESIGN §2 "Robust triangulation"; include/skimi.h).  One workgroup per time step, a
// group of 16 lanes per joint (512 threads at the most: the Jacobi solve wants ~190 VGPRs, which a 1024-thread workgroup
// does not have).  The V (V - 1) / 2 <= 28 two-view hypotheses of a joint are dealt over the group's lanes, two to a lane
// at V >= 7 and one below, each solved and scored against every eligible view, so the hypotheses cost one or two Jacobi
// solves of latency and not 28; the winner (most inliers, then the smaller truncated cost, then the earlier pair: a total
// order, so the butterfly's order does not matter) comes out of four __shfl_xor steps inside the group.  Lane 0 of the
// group then runs what exists once per joint: the refits, the Gauss-Newton steps and the outputs.  The cameras P_v of
// the step, the joint's keypoints and weights live in LDS, where a runtime view index costs nothing; the 4 x 4 arrays
// stay in registers.  After a barrier thread v < V reduces view v's inlier ratio and thread V the step's report, in joint
// order.  No atomics, every sum in a fixed order.
constexpr int kRobustLanes = 16, kRobustMaxIters = 32;

__device__ __forceinline__ int n_bits(int set) { return __popc((unsigned)set); }

struct RobustScore {
    int set;       // bit v: view v is an inlier
    int n;         // popcount(set)
    double cost;   // truncated cost over the eligible views
};

// p = P_v (X, 1), summed left to right
__device__ __forceinline__ void project_view(const double* P, const double (&X)[3], double (&p)[3]) {
#pragma unroll
    for (int a = 0; a < 3; ++a) p[a] = P[a * 4] * X[0] + P[a * 4 + 1] * X[1] + P[a * 4 + 2] * X[2] + P[a * 4 + 3];
}

// rule 3: errors of X in the eligible views, in view order
__device__ __forceinline__ RobustScore robust_score(const double (*sP)[12], const double (*kp)[2], int V, int elig,
                                                    const double (&X)[3], double thr) {
    RobustScore r = {0, 0, 0.0};
#pragma nounroll
    for (int v = 0; v < V; ++v) {
        if (!((elig >> v) & 1)) continue;
        double p[3];
        project_view(sP[v], X, p);
        const double du = p[0] / p[2] - kp[v][0], dv = p[1] / p[2] - kp[v][1];
        const double e = sqrt(du * du + dv * dv);
        const bool front = p[2] > 0;
        if (front && e <= thr) {
            r.set |= 1 << v;
            ++r.n;
        }
        const double c = (front && isfinite(e)) ? (e < thr ? e : thr) : thr;
        r.cost += c * c;
    }
    return r;
}

// rule 8: the weights of a set's refit / refinement; a set with fewer than two positive weights is taken unweighted
__device__ __forceinline__ bool robust_use_weights(const double* w, int V, int set) {
    int n = 0;
    for (int v = 0; v < V; ++v) n += ((set >> v) & 1) && w[v] > 0;
    return n >= 2;
}

// c(X + d) - c(X) for c(X) = sum over the set of w_v^2 ||pi_v(X) - keypoint_v||^2, in view order, formed from the step: with
// u = pi_v(X), r = u - keypoint_v and (a, b) = P_v[:, :3] d the residual moves by dr = (a_xy - u b) / (z + b), and
// |r + dr|^2 - |r|^2 = dr . (2 r + dr).  Two rounded sums c(X + d), c(X) cannot show a decrease under eps c, i.e. a step
// under ~1e-10, and which side of that a step falls on depends on the last bits of X; this difference keeps its sign.
__device__ __forceinline__ double robust_cost_change(const double (*sP)[12], const double (*kp)[2], const double* w,
                                                     bool use_w, int V, int set, const double (&X)[3],
                                                     const double (&d)[3]) {
    double dc = 0;
#pragma nounroll
    for (int v = 0; v < V; ++v) {
        if (!((set >> v) & 1)) continue;
        const double* P = sP[v];
        double p[3];
        project_view(P, X, p);
        const double u0 = p[0] / p[2], u1 = p[1] / p[2];
        const double r0 = u0 - kp[v][0], r1 = u1 - kp[v][1];
        const double a0 = P[0] * d[0] + P[1] * d[1] + P[2] * d[2], a1 = P[4] * d[0] + P[5] * d[1] + P[6] * d[2],
                     b = P[8] * d[0] + P[9] * d[1] + P[10] * d[2];
        const double dr0 = (a0 - u0 * b) / (p[2] + b), dr1 = (a1 - u1 * b) / (p[2] + b);
        const double w2 = use_w ? w[v] * w[v] : 1.0;
        dc += w2 * (dr0 * (2.0 * r0 + dr0) + dr1 * (2.0 * r1 + dr1));
    }
    return dc;
}

__global__ __launch_bounds__(kRobustLanes * kTriageMaxJ) void triangulate_robust_kernel(
    const float* __restrict__ Kc, const float* __restrict__ Rc, const float* __restrict__ tc, const float* __restrict__ kp,
    const float* __restrict__ conf, double conf_thr, double thr, int min_inliers, int refine_iters, int weighted, int V,
    int J, float* __restrict__ X_out, float* __restrict__ Xok_out, double* __restrict__ err,
    unsigned char* __restrict__ inlier_views, double* __restrict__ rms_px, unsigned char* __restrict__ ok_out,
    double* __restrict__ view_ratio, double* __restrict__ report) {
    __shared__ double s_P[kTriageMaxV][12];
    __shared__ double s_kp[kTriageMaxJ][kTriageMaxV][2];
    __shared__ double s_w[kTriageMaxJ][kTriageMaxV];
    __shared__ unsigned char s_flag[kTriageMaxJ][kTriageMaxV];   // bit 0: finite keypoint, bit 1: eligible
    __shared__ double s_rms[kTriageMaxJ];
    __shared__ int s_set[kTriageMaxJ], s_state[kTriageMaxJ];     // state bit 0: did not fail, bit 1: ok
    const long t = blockIdx.x;
    const int tid = threadIdx.x;
    const int j = tid / kRobustLanes, lane = tid % kRobustLanes;
    const bool active = j < J;
    const double nan = __longlong_as_double(0x7FF8000000000000LL);

    for (int i = tid; i < V * 12; i += blockDim.x) {   // P_v = K_v [R_v | t_v], entry by entry as camera_P sums it
        const int v = i / 12, a = (i % 12) / 4, b = i % 4;
        const float* K = Kc + (t * V + v) * 9;
        const float* R = Rc + (t * V + v) * 9;
        const float* tt = tc + (t * V + v) * 3;
        double s = 0;
#pragma unroll
        for (int c = 0; c < 3; ++c) s += (double)K[a * 3 + c] * (b < 3 ? (double)R[c * 3 + b] : (double)tt[c]);
        s_P[v][i % 12] = s;
    }
    if (active && lane < V) {   // rules 1 and 8 for view `lane` of joint j
        const long o = (t * V + lane) * J + j;
        const double u = kp[o * 2], w = kp[o * 2 + 1];
        const bool fin = isfinite(u) && isfinite(w);
        bool elig = fin;
        double wt = 1.0;
        if (conf) {
            const double c = (double)conf[o];
            elig = elig && c >= conf_thr;
            if (weighted) wt = isfinite(c) ? (c < 0 ? 0.0 : (c > 1 ? 1.0 : c)) : 0.0;
        }
        s_kp[j][lane][0] = u;
        s_kp[j][lane][1] = w;
        s_w[j][lane] = wt;
        s_flag[j][lane] = (unsigned char)((fin ? 1 : 0) | (elig ? 2 : 0));
    }
    __syncthreads();

    // ---- rules 2 - 4: the hypotheses, dealt over the lanes; a group beyond J only takes part in the shuffles -----------
    int elig = 0, finite_kp = 0;
    if (active)
        for (int v = 0; v < V; ++v) {
            elig |= ((s_flag[j][v] >> 1) & 1) << v;
            finite_kp |= (s_flag[j][v] & 1) << v;
        }
    // lane l owns the pairs h = l and l + 16 of the V (V - 1) / 2 <= 28 pairs a < b in lexicographic order and keeps the
    // better of its two (the second pass exists at V >= 7 only)
    const int n_pairs = V * (V - 1) / 2;
    int h_n = -1, h_set = 0, h_h = lane;
    double h_cost = 0, hX[3] = {nan, nan, nan};
#pragma nounroll
    for (int h = lane; h - lane < n_pairs; h += kRobustLanes) {
        int va = 0, vb = h;
        while (va < V - 1 && vb >= V - 1 - va) {
            vb -= V - 1 - va;
            ++va;
        }
        vb += va + 1;
        if (!(active && h < n_pairs && ((elig >> va) & 1) && ((elig >> vb) & 1))) continue;
        double M[4][4] = {{0}};
        dlt_add_view<false>(M, s_P[va], s_kp[j][va][0], s_kp[j][va][1], 1.0);
        dlt_add_view<false>(M, s_P[vb], s_kp[j][vb][0], s_kp[j][vb][1], 1.0);
        bool fin = true;
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) fin = fin && isfinite(M[a][b]);
        if (!fin) continue;
        double Xh[3];
        dlt_solve(M, Xh);
        if (!(isfinite(Xh[0]) && isfinite(Xh[1]) && isfinite(Xh[2]))) continue;
        const RobustScore sc = robust_score(s_P, s_kp[j], V, elig, Xh, thr);
        if (sc.n > h_n || (sc.n == h_n && sc.cost < h_cost)) {   // equal keys keep the earlier pair
            h_n = sc.n;
            h_set = sc.set;
            h_cost = sc.cost;
            h_h = h;
            hX[0] = Xh[0];
            hX[1] = Xh[1];
            hX[2] = Xh[2];
        }
    }
    int b_n = h_n, b_h = h_h, b_lane = lane;
    double b_cost = h_cost;
#pragma unroll
    for (int off = kRobustLanes / 2; off > 0; off >>= 1) {
        const int o_n = __shfl_xor(b_n, off, kRobustLanes), o_h = __shfl_xor(b_h, off, kRobustLanes);
        const double o_cost = __shfl_xor(b_cost, off, kRobustLanes);
        const bool better = o_n > b_n || (o_n == b_n && (o_cost < b_cost || (o_cost == b_cost && o_h < b_h)));
        const int o_lane = __shfl_xor(b_lane, off, kRobustLanes);
        if (better) {
            b_n = o_n;
            b_h = o_h;
            b_cost = o_cost;
            b_lane = o_lane;
        }
    }
    double X[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) X[a] = __shfl(hX[a], b_lane, kRobustLanes);
    int set = __shfl(h_set, b_lane, kRobustLanes);

    // ---- rules 5 - 7: once per joint ----------------------------------------------------------------------------------
    if (active && lane == 0) {
        const double(*kpj)[2] = s_kp[j];
        const double* wj = s_w[j];
        const bool failed = b_n < 2;
        double rms = nan;
        if (failed) {
            set = 0;
            X[0] = X[1] = X[2] = nan;
        } else {
#pragma nounroll
            for (int round = 0; round < 3; ++round) {   // rule 5
                const bool use_w = robust_use_weights(wj, V, set);
                double M[4][4] = {{0}};
#pragma nounroll
                for (int v = 0; v < V; ++v)
                    if ((set >> v) & 1) dlt_add_view<true>(M, s_P[v], kpj[v][0], kpj[v][1], use_w ? wj[v] : 1.0);
                double Xn[3];
                dlt_solve(M, Xn);
                const RobustScore sc = robust_score(s_P, kpj, V, elig, Xn, thr);
                if (sc.n < 2) break;
                const bool same = sc.set == set;
                X[0] = Xn[0];
                X[1] = Xn[1];
                X[2] = Xn[2];
                set = sc.set;
                if (same) break;
            }
            if (refine_iters > 0) {   // rule 6
                const bool use_w = robust_use_weights(wj, V, set);
#pragma nounroll
                for (int it = 0; it < refine_iters; ++it) {
                    double H00 = 0, H10 = 0, H11 = 0, H20 = 0, H21 = 0, H22 = 0, g0 = 0, g1 = 0, g2 = 0;
#pragma nounroll
                    for (int v = 0; v < V; ++v) {
                        if (!((set >> v) & 1)) continue;
                        const double* P = s_P[v];
                        double p[3];
                        project_view(P, X, p);
                        const double z = p[2], zz = z * z;
                        const double du = p[0] / z - kpj[v][0], dv = p[1] / z - kpj[v][1];
                        const double a0 = (P[0] * z - p[0] * P[8]) / zz, a1 = (P[1] * z - p[0] * P[9]) / zz,
                                     a2 = (P[2] * z - p[0] * P[10]) / zz;
                        const double b0 = (P[4] * z - p[1] * P[8]) / zz, b1 = (P[5] * z - p[1] * P[9]) / zz,
                                     b2 = (P[6] * z - p[1] * P[10]) / zz;
                        const double w2 = use_w ? wj[v] * wj[v] : 1.0;
                        H00 += w2 * (a0 * a0 + b0 * b0);
                        H10 += w2 * (a1 * a0 + b1 * b0);
                        H11 += w2 * (a1 * a1 + b1 * b1);
                        H20 += w2 * (a2 * a0 + b2 * b0);
                        H21 += w2 * (a2 * a1 + b2 * b1);
                        H22 += w2 * (a2 * a2 + b2 * b2);
                        g0 += w2 * (a0 * du + b0 * dv);
                        g1 += w2 * (a1 * du + b1 * dv);
                        g2 += w2 * (a2 * du + b2 * dv);
                    }
                    // H d = -g by LDL^T, no pivoting
                    const double d0 = H00, l10 = H10 / d0, l20 = H20 / d0;
                    const double d1 = H11 - l10 * l10 * d0;
                    const double l21 = (H21 - l20 * l10 * d0) / d1;
                    const double d2 = H22 - l20 * l20 * d0 - l21 * l21 * d1;
                    const double y0 = -g0, y1 = -g1 - l10 * y0, y2 = -g2 - l20 * y0 - l21 * y1;
                    const double s2 = y2 / d2, s1 = y1 / d1 - l21 * s2, s0 = y0 / d0 - l10 * s1 - l20 * s2;
                    const double Xn[3] = {X[0] + s0, X[1] + s1, X[2] + s2};
                    if (!(isfinite(Xn[0]) && isfinite(Xn[1]) && isfinite(Xn[2]))) break;
                    const double d[3] = {Xn[0] - X[0], Xn[1] - X[1], Xn[2] - X[2]};   // the step X can take
                    if (!(robust_cost_change(s_P, kpj, wj, use_w, V, set, X, d) < 0)) break;
                    X[0] = Xn[0];
                    X[1] = Xn[1];
                    X[2] = Xn[2];
                }
            }
            double sq = 0;
            int n = 0;
#pragma nounroll
            for (int v = 0; v < V; ++v) {   // rule 7: the final errors, of every view with a finite keypoint
                double p[3];
                project_view(s_P[v], X, p);
                const double du = p[0] / p[2] - kpj[v][0], dv = p[1] / p[2] - kpj[v][1];
                const double e = sqrt(du * du + dv * dv);
                err[(t * V + v) * J + j] = ((finite_kp >> v) & 1) ? e : nan;
                if ((set >> v) & 1) {
                    sq += e * e;
                    ++n;
                }
            }
            rms = sqrt(sq / (double)n);
        }
        if (failed)
            for (int v = 0; v < V; ++v) err[(t * V + v) * J + j] = nan;
        const bool ok = !failed && n_bits(set) >= min_inliers && isfinite(X[0]) && isfinite(X[1]) && isfinite(X[2]);
        const float nanf_ = __uint_as_float(0x7FC00000u);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float x = failed ? nanf_ : (float)X[a];
            X_out[(t * J + j) * 3 + a] = x;
            Xok_out[(t * J + j) * 3 + a] = ok ? x : nanf_;
        }
        inlier_views[t * J + j] = (unsigned char)set;
        rms_px[t * J + j] = rms;
        ok_out[t * J + j] = ok ? 1 : 0;
        s_set[j] = set;
        s_rms[j] = rms;
        s_state[j] = (failed ? 0 : 1) | (ok ? 2 : 0);
    }
    __syncthreads();
    if (tid < V) {   // the share of the joints that did not fail which hold view tid in their set
        int n = 0, m = 0;
        for (int i = 0; i < J; ++i) {
            n += s_state[i] & 1;
            m += (s_set[i] >> tid) & 1;   // a failed joint's set is 0
        }
        view_ratio[t * V + tid] = n ? (double)m / (double)n : nan;
    } else if (tid == V) {
        int nok = 0, bits = 0, m = 0;
        double sq = 0;
        for (int i = 0; i < J; ++i) {
            if (!(s_state[i] & 2)) continue;
            ++nok;
            bits += n_bits(s_set[i]);
            const double r = s_rms[i];
            if (r == r) {
                sq += r * r;
                ++m;
            }
        }
        double* o = report + t * 4;
        o[0] = (double)nok;
        o[1] = (double)nok / (double)J;
        o[2] = nok ? (double)bits / (double)nok : nan;
        o[3] = m ? sqrt(sq / (double)m) : nan;
    }
}

}  // namespace skimi

using namespace skimi;

extern "C" {

int skimi_pose_to_cameras(const float* pose_enc, int64_t rows, int32_t H, int32_t W, float* extrinsic, float* intrinsic,
                          void* stream) {
    SKIMI_CHECK_ARG(pose_enc && extrinsic && rows > 0 && H > 0 && W > 0, "skimi_pose_to_cameras: bad arguments");
    hipLaunchKernelGGL(pose_to_cameras_kernel, dim3((unsigned)cdiv(rows, 64)), dim3(64), 0, (hipStream_t)stream, pose_enc,
                       extrinsic, intrinsic, (long)rows, (float)H, (float)W);
    SKIMI_LAUNCH_CHECK();
    return SKIMI_OK;
}

int skimi_unproject_depth(const float* depth, const float* extrinsic, const float* intrinsic, float* world_points,
                          int32_t frames, int32_t H, int32_t W, void* stream) {
    SKIMI_CHECK_ARG(depth && extrinsic && intrinsic && world_points && frames > 0 && H > 0 && W > 0,
                    "skimi_unproject_depth: bad arguments");
    const long total = (long)frames * H * W;
    const int blocks = (int)std::min<long>(cdiv(total, 256), 16384);
    hipLaunchKernelGGL(unproject_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, depth, extrinsic, intrinsic,
                       world_points, frames, H, W);
    SKIMI_LAUNCH_CHECK();
    return SKIMI_OK;
}

int skimi_triangulate_dlt(const float* K, const float* R, const float* t, const float* keypoints, float* joints3d,
                          int64_t steps, int32_t views, int32_t joints, void* stream) {
    SKIMI_CHECK_ARG(K && R && t && keypoints && joints3d && steps > 0 && views >= 2 && joints > 0,
                    "skimi_triangulate_dlt: bad arguments (need >= 2 views)");
    const long n = steps * joints;
    hipLaunchKernelGGL(triangulate_dlt_kernel, dim3((unsigned)cdiv(n, 64)), dim3(64), 0, (hipStream_t)stream, K, R, t,
                       keypoints, joints3d, (long)steps, views, joints);
    SKIMI_LAUNCH_CHECK();
    return SKIMI_OK;
}

int skimi_triangulate_triage(const float* K, const float* R, const float* t, const float* keypoints, const float* conf,
                             double conf_thr, double err_thresh_px, int64_t steps, int32_t views, int32_t joints,
                             float* joints3d, float* joints3d_clean, double* err, double* depth, uint8_t* keep,
                             double* view_stats, double* report, void* stream) {
    SKIMI_CHECK_ARG(K && R && t && keypoints && joints3d && joints3d_clean && err && depth && keep && view_stats && report &&
                        steps > 0 && steps < ((int64_t)1 << 31) && views >= 2 && views <= kTriageMaxV && joints >= 1 &&
                        joints <= kTriageMaxJ,
                    "skimi_triangulate_triage: bad arguments (need 2..8 views, 1..32 joints)");
    hipLaunchKernelGGL(triangulate_triage_kernel, dim3((unsigned)steps), dim3(64), 0, (hipStream_t)stream, K, R, t, keypoints,
                       conf, conf_thr, err_thresh_px, views, joints, joints3d, joints3d_clean, err, depth, keep, view_stats,
                       report);
    SKIMI_LAUNCH_CHECK();
    return SKIMI_OK;
}

int skimi_triangulate_robust(const float* K, const float* R, const float* t, const float* keypoints, const float* conf,
                             double conf_thr, double inlier_px, int32_t min_inliers, int32_t refine_iters, int32_t weighted,
                             int64_t steps, int32_t views, int32_t joints, float* joints3d, double* err,
                             uint8_t* inlier_views, double* rms_px, uint8_t* ok, float* joints3d_ok,
                             double* view_inlier_ratio, double* report, void* stream) {
    SKIMI_CHECK_ARG(K && R && t && keypoints && joints3d && err && inlier_views && rms_px && ok && joints3d_ok &&
                        view_inlier_ratio && report,
                    "skimi_triangulate_robust: null pointer (only conf may be NULL)");
    SKIMI_CHECK_ARG(steps > 0 && steps < ((int64_t)1 << 31) && views >= 2 && views <= kTriageMaxV && joints >= 1 &&
                        joints <= kTriageMaxJ,
                    "skimi_triangulate_robust: bad shape (need steps > 0, 2..8 views, 1..32 joints; got %lld, %d, %d)",
                    (long long)steps, views, joints);
    SKIMI_CHECK_ARG(min_inliers >= 2 && min_inliers <= views, "skimi_triangulate_robust: min_inliers must be in 2..views (%d), got %d",
                    views, min_inliers);
    SKIMI_CHECK_ARG(refine_iters >= 0 && refine_iters <= kRobustMaxIters,
                    "skimi_triangulate_robust: refine_iters must be in 0..32, got %d", refine_iters);
    SKIMI_CHECK_ARG(inlier_px >= 0 && conf_thr == conf_thr && (weighted == 0 || weighted == 1),
                    "skimi_triangulate_robust: inlier_px must be >= 0, conf_thr a number, weighted 0 or 1");
    const int threads = (joints * kRobustLanes + 63) / 64 * 64;
    hipLaunchKernelGGL(triangulate_robust_kernel, dim3((unsigned)steps), dim3(threads), 0, (hipStream_t)stream, K, R, t,
                       keypoints, conf, conf_thr, inlier_px, min_inliers, refine_iters, weighted, views, joints, joints3d,
                       joints3d_ok, err, inlier_views, rms_px, ok, view_inlier_ratio, report);
    SKIMI_LAUNCH_CHECK();
    return SKIMI_OK;
}

}  // extern "C"
