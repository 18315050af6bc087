// Camera-and-points refinement (VideoPose3D/slove_rt_from_3d.py --refine camera_points: the lifter's joints are refined
// together with the cameras, under an optional prior lambda_x that ties them to their start).  A problem is one group: the
// points X [N,3] are cut into consecutive groups of group_size, and all V cameras of a group move together with its points.
//
// One launch, one workgroup per group (one wave up to 64 points, up to 512 threads beyond: that leaves 256 registers a
// lane, which hold the widest pass without scratch; profiles/refine_points.md), runs the mask, the K inference, every Levenberg-Marquardt iteration and the final errors: no host round trip, no allocation, no atomics, no
// cross-workgroup traffic.  The step (H + lam I) delta = -g over all 6 V + 3 n parameters is solved exactly through the
// Schur complement on the points: a point's blocks V_i (3 x 3), g_i and W_iv (6 x 3 per view) are written to the workspace
// by the pass that linearises, and a trial at a new lam is made from them: the reduced camera system S = U + lam I -
// sum W V*^-1 W^T is summed one view pair at a time, thread 0 factors it (LDL^T, in LDS), and one more pass takes every
// point's own step, writes the trial point and sums the change of the cost, formed from the step itself.  A pass
// accumulates per thread in point order (thread i takes the points i, i + threads, ...), then a fixed shuffle tree per
// wave, then the waves in order, so every sum depends only on a point's index within its group.  A point's workspace
// entries are written and read by the same thread only.  All arithmetic is float64.  Rules: DESIGN §2 "Camera + points
// refinement"; restated in tests/refine_restated.py.  The projection and `packed` are camera_lm.h's, shared with
// resect.hip; the workgroup sums are reduce.h's.  The mask, the loss and the acceptance rule are the resection's, written here again.
#include <math.h>

#include "camera_lm.h"
#include "common.h"
#include "reduce.h"
#include "rodrigues.h"

namespace skimi {
namespace {

constexpr int kMaxWaves = 8;
constexpr int kMaxViews = 4;
constexpr int kMinPoints = 6;
constexpr int kMaxGroup = 0x7fffffff / 3;     // a point's offsets 3 i + 2 within its group are 32-bit
constexpr int kRed = 42;                     // the widest reduction: a 6 x 6 block of S and 6 of its right-hand side
constexpr int kDim = 6 * kMaxViews;
constexpr double kTau = 3e-8;                // rule 8
constexpr double kLambdaMin = 1e-9;          // rule 9
// workspace rows, each [N]: V_i (6, packed upper triangle), g_i (3), the trial point (3), then W_iv (18 per view)
constexpr int kWsV = 0, kWsG = 6, kWsX = 9, kWsW = 12;
enum Phase { STOP = 0, STEP = 1, LINEARISE = 2 };

struct RefineArgs {
    const double *X, *x2d, *conf, *K, *R0, *t0;
    double *R, *t, *K_out, *X_opt, *cost0, *cost, *err, *stats, *moved, *ws;
    int32_t *n_evals, *n_used, *success;
    long N, gs;
    int V, soft, max_evals;
    double f_scale, min_conf, lambda_x, sqrt_lx;
};

struct Cam {
    double R[9], R1[9], t[3], K[5];          // R1 = Exp(omega) R of the trial; K: fx, skew, cx, fy, cy
    double d[6], A, B;                       // the step (omega, dt) and Exp's coefficients for it
    double U[21], g[6];
};

// the controller's state, in LDS
struct State {
    Cam cam[kMaxViews];
    double S[kDim * kDim], rhs[kDim];
    double c, c0, csum, lam, hmax, dn2, xn2;   // dn2, xn2: |delta|^2 and |X|^2 of the last trial
    int evals, success, failed, next, first;
};

// rule 1: is point i of the group at `base` used?  From the caller's X, which a masked point keeps.  resect.hip's
// load_point is the same mask and weight with the loads of one view fused in: a fix here belongs there too.
__device__ inline bool point_used(const RefineArgs& a, long base, int i) {
    const double* Xg = a.X + 3 * base;
    bool used = is_fin(Xg[3 * i]) && is_fin(Xg[3 * i + 1]) && is_fin(Xg[3 * i + 2]);
    for (int v = 0; v < a.V; ++v) {
        const double* xg = a.x2d + 2 * (v * a.N + base);
        used = used && is_fin(xg[2 * i]) && is_fin(xg[2 * i + 1]);
        if (a.conf) {
            const double w = clamp_conf((a.conf + (v * a.N + base))[i]);
            used = used && w >= a.min_conf;
        }
    }
    return used;
}
// view v's keypoint and weight of a used point
__device__ inline void load_obs(const RefineArgs& a, long base, int i, int v, double* x, double& w) {
    const double* xg = a.x2d + 2 * (v * a.N + base);
    x[0] = xg[2 * i];
    x[1] = xg[2 * i + 1];
    w = 1.0;
    if (a.conf) w = clamp_conf((a.conf + (v * a.N + base))[i]);
}
__device__ inline void load3(const double* p, int i, double* X) {
    X[0] = p[3 * i];
    X[1] = p[3 * i + 1];
    X[2] = p[3 * i + 2];
}

// rule 4's loss of one residual component: rho' and the cost's summand (before the factor 1/2 or 1/2 f^2).  resect.hip has
// the same arithmetic inline in its linearisation, and summand_change's in its trial pass: a fix here belongs there too.
__device__ inline double rho1_of(int soft, double f_scale, double r, double& summand) {
    if (soft) {
        const double sq = sqrt(1.0 + (r / f_scale) * (r / f_scale));
        summand = 2.0 * (sq - 1.0);
        return 1.0 / sq;
    }
    summand = r * r;
    return 1.0;
}
// the change of a component's summand when its residual r changes by dr, formed from dr itself
__device__ inline double summand_change(int soft, double f_scale, double r, double dr) {
    const double e = dr * (2.0 * r + dr);
    if (!soft) return e;
    const double z0 = (r / f_scale) * (r / f_scale), dz = e / (f_scale * f_scale);
    return 2.0 * dz / (sqrt(1.0 + (z0 + dz)) + sqrt(1.0 + z0));
}

// V* = V_i + lam I (packed upper triangle xx, xy, xz, yy, yz, zz) as L D L^T without pivoting, and its solves
struct Ldl3 {
    double d0, d1, d2, l10, l20, l21;
};
__device__ inline void factor3(const double* Vp, double lam, Ldl3& f) {
    f.d0 = Vp[0] + lam;
    f.l10 = Vp[1] / f.d0;
    f.l20 = Vp[2] / f.d0;
    f.d1 = (Vp[3] + lam) - f.l10 * f.l10 * f.d0;
    f.l21 = (Vp[4] - f.l20 * f.l10 * f.d0) / f.d1;
    f.d2 = ((Vp[5] + lam) - f.l20 * f.l20 * f.d0) - f.l21 * f.l21 * f.d1;
}
__device__ inline void solve3(const Ldl3& f, const double* b, double* x) {
    const double y0 = b[0], y1 = b[1] - f.l10 * y0, y2 = (b[2] - f.l20 * y0) - f.l21 * y1;
    x[2] = y2 / f.d2;
    x[1] = y1 / f.d1 - f.l21 * x[2];
    x[0] = (y0 / f.d0 - f.l10 * x[1]) - f.l20 * x[2];
}

// One pass of the linearisation of view v over the group's used points.  kPoint: the point blocks (V_i and g_i gain this
// view's part, W_iv is written), the camera gradient and the cost (7 sums); rows kRow0 .. kRow1 - 1 of the upper
// triangle of U_v are summed besides.  `take`: the points first move to their accepted trial position (view 0's kPoint pass
// only).  Returns the thread's largest diagonal entry of V_i (kPoint passes).
template <int kRow0, int kRow1, bool kPoint>
__device__ inline double linearise_pass(const RefineArgs& a, State& s, long base, int gs, int v, bool take, double (*red)[kRed]) {
    constexpr int kU = packed(kRow1 - 1, 5) + 1 - packed(kRow0, kRow0);       // rows are consecutive in the packing
    constexpr int kAcc = (kRow1 > kRow0 ? kU : 0) + (kPoint ? 7 : 0);
    constexpr int kU0 = kRow1 > kRow0 ? packed(kRow0, kRow0) : 0, kG = kRow1 > kRow0 ? kU : 0;
    const int tid = threadIdx.x, nt = blockDim.x;
    const Cam& cam = s.cam[v];
    double* Xo = a.X_opt + 3 * base;
    double* ws = a.ws + base;
    const long N = a.N;
    double acc[kAcc], hmax = 0.0;
#pragma unroll
    for (int k = 0; k < kAcc; ++k) acc[k] = 0.0;
    for (int i = tid; i < gs; i += nt) {
        if (!point_used(a, base, i)) continue;
        double X[3], x[2], w;
        if (kPoint && take) {
#pragma unroll
            for (int k = 0; k < 3; ++k) Xo[3 * i + k] = X[k] = ws[(kWsX + k) * N + i];
        } else {
            load3(Xo, i, X);
        }
        load_obs(a, base, i, v, x, w);
        Proj pr;
        residual(cam, X, x, w, pr);
        // the x component, then the y component: J = [q x a, a] over the camera, a R over the point, a = d r / d Xc
        double Jc[2][6], Jp[2][3], rho1[2];
        Jc[0][3] = w * (cam.K[0] / pr.z), Jc[0][4] = w * (cam.K[1] / pr.z), Jc[0][5] = w * (-pr.pu / pr.z);
        Jc[1][3] = 0.0, Jc[1][4] = w * (cam.K[3] / pr.z), Jc[1][5] = w * (-(cam.K[3] * pr.v) / pr.z);
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            cross3(pr.q, Jc[c] + 3, Jc[c]);
            double summand;
            rho1[c] = rho1_of(a.soft, a.f_scale, pr.r[c], summand);
            if (kPoint) acc[kG + 6] += summand;
            if (kRow1 > kRow0) {
#pragma unroll
                for (int i0 = kRow0; i0 < kRow1; ++i0)
#pragma unroll
                    for (int i1 = i0; i1 < 6; ++i1) acc[packed(i0, i1) - kU0] += rho1[c] * (Jc[c][i0] * Jc[c][i1]);
            }
            if (kPoint) {
#pragma unroll
                for (int k = 0; k < 6; ++k) acc[kG + k] += rho1[c] * (Jc[c][k] * pr.r[c]);
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    Jp[c][k] = (Jc[c][3] * cam.R[k] + Jc[c][4] * cam.R[3 + k]) + Jc[c][5] * cam.R[6 + k];
            }
        }
        if (kPoint) {
            double Vp[6], gp[3];
            if (v == 0) {
                // the prior's three components (rule 4), or nothing
#pragma unroll
                for (int k = 0; k < 6; ++k) Vp[k] = 0.0;
                gp[0] = gp[1] = gp[2] = 0.0;
                if (a.lambda_x > 0.0) {
                    double X0[3];
                    load3(a.X + 3 * base, i, X0);
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        const double rp = a.sqrt_lx * (X[k] - X0[k]);
                        double summand;
                        const double rh = rho1_of(a.soft, a.f_scale, rp, summand);
                        acc[kG + 6] += summand;
                        Vp[k == 0 ? 0 : k == 1 ? 3 : 5] = rh * (a.sqrt_lx * a.sqrt_lx);
                        gp[k] = rh * (a.sqrt_lx * rp);
                    }
                }
            } else {
#pragma unroll
                for (int k = 0; k < 6; ++k) Vp[k] = ws[(kWsV + k) * N + i];
#pragma unroll
                for (int k = 0; k < 3; ++k) gp[k] = ws[(kWsG + k) * N + i];
            }
            int m = 0;
#pragma unroll
            for (int i0 = 0; i0 < 3; ++i0) {
#pragma unroll
                for (int i1 = i0; i1 < 3; ++i1)
                    Vp[m++] += rho1[0] * (Jp[0][i0] * Jp[0][i1]) + rho1[1] * (Jp[1][i0] * Jp[1][i1]);
                gp[i0] += rho1[0] * (Jp[0][i0] * pr.r[0]) + rho1[1] * (Jp[1][i0] * pr.r[1]);
            }
#pragma unroll
            for (int k = 0; k < 6; ++k) ws[(kWsV + k) * N + i] = Vp[k];
#pragma unroll
            for (int k = 0; k < 3; ++k) ws[(kWsG + k) * N + i] = gp[k];
            double* W = ws + (kWsW + 18 * v) * N;
#pragma unroll
            for (int r = 0; r < 6; ++r)
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    W[(3 * r + k) * N + i] = rho1[0] * (Jc[0][r] * Jp[0][k]) + rho1[1] * (Jc[1][r] * Jp[1][k]);
            hmax = fmax(hmax, fmax(Vp[0], fmax(Vp[3], Vp[5])));
        }
    }
    block_sum<kAcc>(acc, red);
    if (tid == 0) {
        Cam& cw = s.cam[v];
        if (kRow1 > kRow0)
            for (int k = 0; k < kU; ++k) cw.U[kU0 + k] = total(red, k);
        if (kPoint) {
            for (int k = 0; k < 6; ++k) cw.g[k] = total(red, kG + k);
            s.csum = v == 0 ? total(red, kG + 6) : s.csum + total(red, kG + 6);
        }
    }
    return hmax;
}

// Rows kA0 .. kA1 - 1 of the 6 x 6 block sum_i W_iv1 V*_i^-1 W_iv2^T of S (v2 <= v1: the lower triangle, which the
// LDL^T reads), and on the diagonal blocks the same rows of sum_i W_iv1 V*_i^-1 g_i
template <int kA0, int kA1>
__device__ inline void schur_pass(const RefineArgs& a, State& s, long base, int gs, int v1, int v2, double (*red)[kRed]) {
    constexpr int kA = kA1 - kA0;
    const int tid = threadIdx.x, nt = blockDim.x;
    const double* ws = a.ws + base;
    const long N = a.N;
    const double lam = s.lam;
    double acc[7 * kA];
#pragma unroll
    for (int k = 0; k < 7 * kA; ++k) acc[k] = 0.0;
    for (int i = tid; i < gs; i += nt) {
        if (!point_used(a, base, i)) continue;
        double Vp[6], gp[3], W2[18];
#pragma unroll
        for (int k = 0; k < 6; ++k) Vp[k] = ws[(kWsV + k) * N + i];
#pragma unroll
        for (int k = 0; k < 3; ++k) gp[k] = ws[(kWsG + k) * N + i];
        Ldl3 f;
        factor3(Vp, lam, f);
        const double *W1p = ws + (kWsW + 18 * v1) * N, *W2p = ws + (kWsW + 18 * v2) * N;
#pragma unroll
        for (int k = 0; k < 18; ++k) W2[k] = W2p[k * N + i];
#pragma unroll
        for (int r = 0; r < kA; ++r) {
            double wr[3], y[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) wr[k] = W1p[(3 * (kA0 + r) + k) * N + i];
            solve3(f, wr, y);
#pragma unroll
            for (int b = 0; b < 6; ++b) acc[6 * r + b] += (y[0] * W2[3 * b] + y[1] * W2[3 * b + 1]) + y[2] * W2[3 * b + 2];
            acc[6 * kA + r] += (y[0] * gp[0] + y[1] * gp[1]) + y[2] * gp[2];
        }
    }
    block_sum<7 * kA>(acc, red);
    if (tid == 0) {
        for (int r = 0; r < kA; ++r) {
            const int row = 6 * v1 + kA0 + r;
            for (int b = 0; b < 6; ++b) s.S[row * kDim + 6 * v2 + b] = total(red, 6 * r + b);
            if (v1 == v2) s.rhs[row] = total(red, 6 * kA + r);
        }
    }
}

// thread 0: S and rhs from the sums, delta_c = S^-1 rhs by LDL^T without pivoting (in place: L below the diagonal, D on
// it), then every view's step, Exp's coefficients and trial rotation
__device__ __forceinline__ void solve_cameras(State& s, int V) {
    const int n = 6 * V;
    double* S = s.S;
    for (int v = 0; v < V; ++v)
        for (int r = 0; r < 6; ++r) {
            const int row = 6 * v + r;
            for (int c = 0; c <= row; ++c) {
                double e = -S[row * kDim + c];
                if (c >= 6 * v) e = (s.cam[v].U[packed(r, c - 6 * v)] + (c == row ? s.lam : 0.0)) + e;
                S[row * kDim + c] = e;
            }
            s.rhs[row] = -s.cam[v].g[r] + s.rhs[row];
        }
    for (int j = 0; j < n; ++j) {
        double d = S[j * kDim + j];
        for (int k = 0; k < j; ++k) d -= S[j * kDim + k] * S[j * kDim + k] * S[k * kDim + k];
        S[j * kDim + j] = d;
        for (int i = j + 1; i < n; ++i) {
            double e = S[i * kDim + j];
            for (int k = 0; k < j; ++k) e -= S[i * kDim + k] * S[j * kDim + k] * S[k * kDim + k];
            S[i * kDim + j] = e / d;
        }
    }
    double* y = s.rhs;
    for (int i = 0; i < n; ++i) {
        double e = y[i];
        for (int k = 0; k < i; ++k) e -= S[i * kDim + k] * y[k];
        y[i] = e;
    }
    for (int i = 0; i < n; ++i) y[i] = y[i] / S[i * kDim + i];
    for (int i = n - 1; i >= 0; --i) {
        double e = y[i];
        for (int k = i + 1; k < n; ++k) e -= S[k * kDim + i] * y[k];
        y[i] = e;
    }
    double dn2 = 0.0;
    for (int v = 0; v < V; ++v) {
        Cam& c = s.cam[v];
        for (int k = 0; k < 6; ++k) {
            c.d[k] = y[6 * v + k];
            dn2 += c.d[k] * c.d[k];
        }
        Rot r;
        rodrigues(c.d, r);
        c.A = r.A;
        c.B = r.B;
        rotate(r, c.R, c.R1);
    }
    s.dn2 = dn2;
}

// every point's own step dX_i = -V*_i^-1 (g_i + sum_v W_iv^T delta_v), the trial point, and the sums of rule 7 and 8:
// the change of the cost's summands, |dX|^2 and |X + dX|^2
__device__ inline void trial_pass(const RefineArgs& a, State& s, long base, int gs, double (*red)[kRed]) {
    const int tid = threadIdx.x, nt = blockDim.x;
    double* ws = a.ws + base;
    const double* Xo = a.X_opt + 3 * base;
    const long N = a.N;
    const double lam = s.lam;
    double acc[3] = {0.0, 0.0, 0.0};
    for (int i = tid; i < gs; i += nt) {
        if (!point_used(a, base, i)) continue;
        double Vp[6], b[3], X[3], dX[3], Xn[3];
#pragma unroll
        for (int k = 0; k < 6; ++k) Vp[k] = ws[(kWsV + k) * N + i];
#pragma unroll
        for (int k = 0; k < 3; ++k) b[k] = ws[(kWsG + k) * N + i];
        for (int v = 0; v < a.V; ++v) {
            const double* W = ws + (kWsW + 18 * v) * N;
            const Cam& cam = s.cam[v];
#pragma unroll
            for (int r = 0; r < 6; ++r)
#pragma unroll
                for (int k = 0; k < 3; ++k) b[k] += W[(3 * r + k) * N + i] * cam.d[r];
        }
        Ldl3 f;
        factor3(Vp, lam, f);
        solve3(f, b, dX);
        load3(Xo, i, X);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            Xn[k] = X[k] + -dX[k];
            dX[k] = Xn[k] - X[k];                  // the step X can take
            ws[(kWsX + k) * N + i] = Xn[k];
            acc[1] += dX[k] * dX[k];
            acc[2] += Xn[k] * Xn[k];
        }
        if (a.lambda_x > 0.0) {
            double X0[3];
            load3(a.X + 3 * base, i, X0);
#pragma unroll
            for (int k = 0; k < 3; ++k) acc[0] += summand_change(a.soft, a.f_scale, a.sqrt_lx * (X[k] - X0[k]), a.sqrt_lx * dX[k]);
        }
        for (int v = 0; v < a.V; ++v) {
            const Cam& cam = s.cam[v];
            double x[2], w, c1[3], c2[3], d[3];
            load_obs(a, base, i, v, x, w);
            Proj pr;
            residual(cam, X, x, w, pr);
            cross3(cam.d, pr.q, c1);
            cross3(cam.d, c1, c2);
#pragma unroll
            for (int k = 0; k < 3; ++k)
                d[k] = ((cam.A * c1[k] + cam.B * c2[k]) + ((cam.R1[3 * k] * dX[0] + cam.R1[3 * k + 1] * dX[1]) + cam.R1[3 * k + 2] * dX[2])) + cam.d[3 + k];
            const double z1 = pr.z + d[2];
            const double du = (d[0] - pr.u * d[2]) / z1, dv = (d[1] - pr.v * d[2]) / z1;
            acc[0] += summand_change(a.soft, a.f_scale, pr.r[0], w * (cam.K[0] * du + cam.K[1] * dv));
            acc[0] += summand_change(a.soft, a.f_scale, pr.r[1], w * (cam.K[3] * dv));
        }
    }
    block_sum<3>(acc, red);
}

template <int kThreads>
__global__ __launch_bounds__(kThreads) void refine_kernel(RefineArgs a) {
    __shared__ double red[2][kMaxWaves][kRed];
    __shared__ double smax[kMaxWaves];
    __shared__ State s;
    const int tid = threadIdx.x, nt = blockDim.x;
    const long g = blockIdx.x;
    const long base = g * a.gs;
    const int gs = (int)a.gs;
    const int V = a.V;
    const double nan = qnan();

    // ---- X_opt starts as X, bit for bit (an unused point and a failed group keep it); rule 1's count ----
    {
        const unsigned long long* src = reinterpret_cast<const unsigned long long*>(a.X + 3 * base);
        unsigned long long* dst = reinterpret_cast<unsigned long long*>(a.X_opt + 3 * base);
        double acc[1] = {0.0};
        for (int i = tid; i < gs; i += nt) {
#pragma unroll
            for (int k = 0; k < 3; ++k) dst[3 * i + k] = src[3 * i + k];
            if (point_used(a, base, i)) acc[0] += 1.0;
        }
        block_sum<1>(acc, red[0]);
    }
    const double n = total(red[0], 0);
    if (tid == 0) {
        s.failed = n < kMinPoints ? 1 : 0;
        s.evals = 0;
        s.success = 0;
        s.first = 1;
        s.c = s.c0 = nan;
        for (int v = 0; v < V; ++v) {
            double* K = s.cam[v].K;
            if (a.K) {
                const double* Kv = a.K + 9 * v;
                K[0] = Kv[0], K[1] = Kv[1], K[2] = Kv[2], K[3] = Kv[4], K[4] = Kv[5];
            } else {
                K[0] = K[2] = K[3] = K[4] = nan;
                K[1] = 0.0;
            }
        }
    }
    __syncthreads();
    bool failed = n < kMinPoints;
    if (!failed) {
        // ---- rule 2: every view's K from its keypoints' spread (the means, then the population std in a second pass) ----
        if (!a.K) {
#pragma unroll 1
            for (int v = 0; v < V; ++v) {
                double acc[2] = {0.0, 0.0};
                for (int i = tid; i < gs; i += nt)
                    if (point_used(a, base, i)) {
                        double x[2], w;
                        load_obs(a, base, i, v, x, w);
                        acc[0] += x[0];
                        acc[1] += x[1];
                    }
                block_sum<2>(acc, red[1]);
                const double cx = total(red[1], 0) / n, cy = total(red[1], 1) / n;
                acc[0] = acc[1] = 0.0;
                for (int i = tid; i < gs; i += nt)
                    if (point_used(a, base, i)) {
                        double x[2], w;
                        load_obs(a, base, i, v, x, w);
                        acc[0] += (x[0] - cx) * (x[0] - cx);
                        acc[1] += (x[1] - cy) * (x[1] - cy);
                    }
                block_sum<2>(acc, red[0]);
                if (tid == 0) {
                    const double sx = sqrt(total(red[0], 0) / n) + 1e-6, sy = sqrt(total(red[0], 1) / n) + 1e-6;
                    s.cam[v].K[0] = s.cam[v].K[3] = 2.0 * fmax(sx, sy);
                    s.cam[v].K[2] = cx;
                    s.cam[v].K[4] = cy;
                }
            }
        }
        // ---- rule 3: the start ----
        for (int k = tid; k < 9 * V; k += nt) s.cam[k / 9].R[k % 9] = a.R0[9 * (g * V) + k];
        for (int k = tid; k < 3 * V; k += nt) s.cam[k / 3].t[k % 3] = a.t0[3 * (g * V) + k];
        __syncthreads();

        // ---- rules 4 to 9: Levenberg-Marquardt; thread 0 decides between the passes ----
        int phase = LINEARISE, buf = 0;
        bool take = false;
        while (phase != STOP) {
            if (phase == LINEARISE) {
                double hmax = 0.0;
#pragma unroll 1
                for (int v = 0; v < V; ++v) {
                    hmax = fmax(hmax, linearise_pass<0, 6, true>(a, s, base, gs, v, take && v == 0, red[buf]));
                    buf ^= 1;
                }
                take = true;
                hmax = block_max(hmax, smax, false);
                if (tid == 0) {
                    for (int v = 0; v < V; ++v)
                        for (int i0 = 0; i0 < 6; ++i0) hmax = fmax(hmax, s.cam[v].U[packed(i0, i0)]);
                    s.hmax = hmax;
                    s.c = (a.soft ? 0.5 * (a.f_scale * a.f_scale) : 0.5) * s.csum;
                    bool ok = is_fin(s.c);
                    int next = STEP;
                    if (s.first) {
                        for (int v = 0; v < V; ++v) {
                            for (int k = 0; k < 9; ++k) ok = ok && is_fin(s.cam[v].R[k]);
                            for (int k = 0; k < 3; ++k) ok = ok && is_fin(s.cam[v].t[k]);
                        }
                        s.first = 0;
                        s.c0 = s.c;
                        s.evals = 1;
                        s.lam = 1e-3 * hmax;
                        if (!ok) {
                            s.failed = 1;
                            next = STOP;
                        }
                    } else if (!ok) {
                        next = STOP;
                    } else {
                        s.lam = fmax(s.lam / 10.0, kLambdaMin * hmax);
                        // rule 8 on the step just accepted
                        double tn2 = s.xn2;
                        for (int v = 0; v < V; ++v)
                            for (int k = 0; k < 3; ++k) tn2 += s.cam[v].t[k] * s.cam[v].t[k];
                        if (sqrt(s.dn2) <= kTau * (1.0 + sqrt(tn2))) {
                            s.success = 1;
                            next = STOP;
                        }
                    }
                    if (next == STEP && s.evals >= a.max_evals) next = STOP;
                    s.next = next;
                }
            } else {
                // ---- a trial at s.lam from the stored blocks ----
#pragma unroll 1
                for (int v1 = 0; v1 < V; ++v1)
#pragma unroll 1
                    for (int v2 = 0; v2 <= v1; ++v2) {
                        schur_pass<0, 6>(a, s, base, gs, v1, v2, red[buf]);
                        buf ^= 1;
                    }
                if (tid == 0) {
                    solve_cameras(s, V);
                    s.evals = s.evals + 1;
                }
                __syncthreads();
                trial_pass(a, s, base, gs, red[buf]);
                if (tid == 0) {
                    const double(*rd)[kRed] = red[buf];
                    const double dc = (a.soft ? 0.5 * (a.f_scale * a.f_scale) : 0.5) * total(rd, 0);
                    int next = STEP;
                    if (is_fin(dc) && dc <= 1e-14 * s.c) {            // c + dc <= c (1 + 1e-14)
                        for (int v = 0; v < V; ++v) {
                            Cam& c = s.cam[v];
                            for (int k = 0; k < 9; ++k) c.R[k] = c.R1[k];
                            for (int k = 0; k < 3; ++k) c.t[k] = c.t[k] + c.d[3 + k];
                        }
                        s.dn2 = s.dn2 + total(rd, 1);
                        s.xn2 = total(rd, 2);
                        next = LINEARISE;
                    } else {
                        s.lam = 10.0 * s.lam;
                        if (!(s.lam < 1e30)) {
                            s.success = 1;
                            next = STOP;
                        } else if (s.evals >= a.max_evals) {
                            next = STOP;
                        }
                    }
                    s.next = next;
                }
                buf ^= 1;
            }
            __syncthreads();
            phase = s.next;
        }
        failed = s.failed != 0;
    }

    // ---- rule 10: the final errors at X_opt, a view at a time, and the group's record ----
    __syncthreads();                           // the controller's last reads of red are done
#pragma unroll 1
    for (int v = 0; v < V; ++v) {
        const Cam& cam = s.cam[v];
        double acc[3] = {0.0, 0.0, 0.0}, emax = 0.0;
        for (int i = tid; i < gs; i += nt) {
            double e = nan;
            if (point_used(a, base, i) && !failed) {
                double X[3], x[2], w;
                load3(a.X_opt + 3 * base, i, X);
                load_obs(a, base, i, v, x, w);
                Proj pr;
                residual(cam, X, x, w, pr);
                const double dx = (pr.pu + cam.K[2]) - x[0], dy = (cam.K[3] * pr.v + cam.K[4]) - x[1];
                e = sqrt(dx * dx + dy * dy);
                acc[0] += e;
                acc[1] += e * e;
                emax = max_nan(emax, e);
                if (v == 0) {
                    double X0[3];
                    load3(a.X + 3 * base, i, X0);
                    acc[2] += ((X[0] - X0[0]) * (X[0] - X0[0]) + (X[1] - X0[1]) * (X[1] - X0[1])) + (X[2] - X0[2]) * (X[2] - X0[2]);
                }
            }
            (a.err + (v * a.N + base))[i] = e;
        }
        emax = block_max(emax, smax, true);
        block_sum<3>(acc, red[v & 1]);
        if (tid == 0) {
            const double(*rd)[kRed] = red[v & 1];
            const long p = g * V + v;
            for (int k = 0; k < 9; ++k) a.R[9 * p + k] = failed ? nan : cam.R[k];
            for (int k = 0; k < 3; ++k) a.t[3 * p + k] = failed ? nan : cam.t[k];
            double* K = a.K_out + 9 * p;
            K[0] = cam.K[0], K[1] = cam.K[1], K[2] = cam.K[2], K[3] = 0.0, K[4] = cam.K[3], K[5] = cam.K[4], K[6] = 0.0, K[7] = 0.0, K[8] = 1.0;
            if (!a.K && n < kMinPoints)
                for (int k = 0; k < 9; ++k) K[k] = nan;
            a.stats[3 * p] = failed ? nan : total(rd, 0) / n;
            a.stats[3 * p + 1] = failed ? nan : sqrt(total(rd, 1) / n);
            a.stats[3 * p + 2] = failed ? nan : emax;
            if (v == 0) a.moved[g] = failed ? nan : sqrt(total(rd, 2) / n);
        }
    }
    if (tid == 0) {
        a.cost0[g] = failed ? nan : s.c0;
        a.cost[g] = failed ? nan : s.c;
        a.n_evals[g] = failed ? 0 : s.evals;
        a.n_used[g] = (int32_t)n;
        a.success[g] = failed ? 0 : s.success;
    }
}

}  // namespace
}  // namespace skimi

using namespace skimi;

extern "C" {

size_t skimi_refine_workspace_bytes(int64_t n_points, int32_t views, int64_t group_size) {
    if (n_points < 1 || views < 1 || views > kMaxViews || n_points > (1LL << 40)) return 0;
    if (group_size < 1 || group_size > kMaxGroup || group_size > n_points || n_points % group_size != 0) return 0;
    return (size_t)(kWsW + 18 * views) * (size_t)n_points * sizeof(double);
}

int skimi_refine_cameras_points(const double* X, const double* x2d, const double* conf, const double* K, const double* R0,
                                const double* t0, int64_t n_points, int32_t views, int64_t group_size, double lambda_x,
                                int32_t loss, double f_scale, double min_conf, int32_t max_evals, double* R, double* t,
                                double* K_out, double* X_opt, double* cost0, double* cost, int32_t* n_evals, int32_t* n_used,
                                int32_t* success, double* err, double* stats, double* moved, void* ws, size_t ws_bytes,
                                void* stream) {
    SKIMI_CHECK_ARG(X && x2d, "skimi_refine_cameras_points: NULL input");
    SKIMI_CHECK_ARG(R && t && K_out && X_opt && cost0 && cost && n_evals && n_used && success && err && stats && moved,
                    "skimi_refine_cameras_points: NULL output");
    SKIMI_CHECK_ARG(X_opt != X, "skimi_refine_cameras_points: X_opt must not be X (the prior and the mask read X throughout)");
    SKIMI_CHECK_ARG(views >= 1 && views <= kMaxViews, "skimi_refine_cameras_points: %d views outside 1..%d", views, kMaxViews);
    SKIMI_CHECK_ARG(n_points >= 1 && group_size >= 1 && group_size <= n_points && n_points % group_size == 0,
                    "skimi_refine_cameras_points: group_size = %lld does not divide n_points = %lld", (long long)group_size,
                    (long long)n_points);
    SKIMI_CHECK_ARG(group_size <= kMaxGroup, "skimi_refine_cameras_points: group_size = %lld above %d (32-bit point offsets)",
                    (long long)group_size, kMaxGroup);
    SKIMI_CHECK_ARG(R0 && t0, "skimi_refine_cameras_points: NULL start (R0, t0 are required)");
    const int64_t groups = n_points / group_size;
    SKIMI_CHECK_ARG(groups * views <= 0x7fffffffLL && n_points <= (1LL << 40),
                    "skimi_refine_cameras_points: %lld groups or %lld points are too many", (long long)groups, (long long)n_points);
    SKIMI_CHECK_ARG(lambda_x >= 0.0 && lambda_x <= 1.79769313486231570815e308,
                    "skimi_refine_cameras_points: lambda_x = %g is not a non-negative number", lambda_x);
    SKIMI_CHECK_ARG(loss == SKIMI_RESECT_LINEAR || loss == SKIMI_RESECT_SOFT_L1, "skimi_refine_cameras_points: unknown loss %d", loss);
    SKIMI_CHECK_ARG(f_scale > 0.0 && f_scale <= 1.79769313486231570815e308,
                    "skimi_refine_cameras_points: f_scale = %g is not a positive number", f_scale);
    SKIMI_CHECK_ARG(min_conf == min_conf, "skimi_refine_cameras_points: min_conf is NaN");
    SKIMI_CHECK_ARG(max_evals >= 1, "skimi_refine_cameras_points: max_evals = %d < 1", max_evals);
    SKIMI_CHECK_ARG(ws && ws_bytes >= skimi_refine_workspace_bytes(n_points, views, group_size),
                    "skimi_refine_cameras_points: workspace of %zu bytes, need %zu", ws_bytes,
                    skimi_refine_workspace_bytes(n_points, views, group_size));
    RefineArgs a{};
    a.X = X, a.x2d = x2d, a.conf = conf, a.K = K, a.R0 = R0, a.t0 = t0;
    a.R = R, a.t = t, a.K_out = K_out, a.X_opt = X_opt, a.cost0 = cost0, a.cost = cost, a.err = err, a.stats = stats;
    a.moved = moved, a.ws = (double*)ws;
    a.n_evals = n_evals, a.n_used = n_used, a.success = success;
    a.N = n_points, a.gs = group_size, a.V = views, a.soft = loss == SKIMI_RESECT_SOFT_L1, a.max_evals = max_evals;
    a.f_scale = f_scale, a.min_conf = min_conf, a.lambda_x = lambda_x, a.sqrt_lx = sqrt(lambda_x);
    hipStream_t st = (hipStream_t)stream;
    if (group_size <= 64) {
        hipLaunchKernelGGL(refine_kernel<64>, dim3((unsigned)groups), dim3(64), 0, st, a);
    } else {
        const int threads = (int)(group_size >= 512 ? 512 : (group_size + 63) / 64 * 64);
        hipLaunchKernelGGL(refine_kernel<512>, dim3((unsigned)groups), dim3(threads), 0, st, a);
    }
    SKIMI_LAUNCH_CHECK();
    return SKIMI_OK;
}

}  // extern "C"
