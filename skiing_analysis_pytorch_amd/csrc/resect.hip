// Camera resection from 3D points and their 2D keypoints (VideoPose3D/slove_rt_from_3d.py: the lifter's joints and both
// views' keypoints -> each camera's (R, t), then the pair's relative pose).  A problem is one (group, view) pair: the
// points X [N,3] are cut into consecutive groups of group_size, and every view of a group is solved on its own.
//
// One launch, one workgroup per problem (one wave up to 64 points, up to 1024 threads beyond), runs the mask, the K
// inference, the DLT initialisation, every Levenberg-Marquardt iteration and the final errors: no host round trip, no
// allocation, no atomics, no cross-workgroup traffic.  A pass over the group's points accumulates per thread in point
// order (thread i takes the points i, i + threads, ...), then a fixed shuffle tree per wave, then the waves in order, so
// every sum depends only on a point's index within its group: a group's results are bitwise the same wherever the group
// sits and whatever else is in the call.  Thread 0 is the controller between passes (6 x 6 LDL^T, Exp, the accept / stop
// rules); its state (R, t, H, g, the step) lives in LDS, as do the 12 x 12 DLT matrix and its eigenvectors, whose cyclic
// Jacobi runs over 12 lanes.  All arithmetic is float64.  Rules: DESIGN §2 "Resection"; restated in
// tests/resect_restated.py.  The projection and `packed` are camera_lm.h's, shared with refine.hip; the workgroup sums are
// reduce.h's.  The mask (load_point), the soft-L1 loss (inline in both passes) and the final maximum are written here and
// again in refine.hip: each spot says so.
#include <math.h>

#include "camera_lm.h"
#include "common.h"
#include "reduce.h"
#include "rodrigues.h"

namespace skimi {
namespace {

constexpr int kMaxWaves = 16;
constexpr int kMaxViews = 8;
constexpr int kMinPoints = 6;
constexpr int kMaxGroup = 0x7fffffff / 3;     // a point's offsets 3 i + 2 within its group are 32-bit
constexpr int kRed = 28;                     // the widest reduction: 21 of H, 6 of g, the cost
constexpr int kJacobiSweeps = 60;
enum Phase { STOP = 0, TRIAL = 1, LINEARISE = 2 };

struct ResectArgs {
    const double *X, *x2d, *conf, *K, *R0, *t0;
    double *R, *t, *K_out, *cost0, *cost, *err, *stats;
    int32_t *n_evals, *n_used, *success;
    long N, gs;
    int V, soft, max_evals;
    double f_scale, min_conf;
};

// the controller's state, in LDS
struct State {
    double R[9], t[3], K[5];                 // K: fx, skew, cx, fy, cy
    double d[6], A, B;                       // the step (omega, dt) and Exp's coefficients for it
    double H[21], g[6], c, c0, lam;
    int evals, success, failed, next, first;
};

// rule 1: point i of the group at `base` with view v's keypoint and weight; false if any view masks it.  The group's
// bases are uniform and i is a 32-bit index, so the addresses cost no 64-bit vector registers.  The same mask and weight
// as refine.hip's point_used + load_obs, kept as a second copy: built from that pair this kernel's assembly changes, and
// its bits and time have not been compared against this form (profiles/shared_device_helpers.md).  A fix here belongs
// there too.
__device__ inline bool load_point(const ResectArgs& a, long base, int i, int v, double* X, double* x, double& w) {
    const double* Xg = a.X + 3 * base;
    X[0] = Xg[3 * i];
    X[1] = Xg[3 * i + 1];
    X[2] = Xg[3 * i + 2];
    bool used = is_fin(X[0]) && is_fin(X[1]) && is_fin(X[2]);
    w = 1.0;
    for (int vv = 0; vv < a.V; ++vv) {
        const double* xg = a.x2d + 2 * (vv * a.N + base);
        const double x0 = xg[2 * i], x1 = xg[2 * i + 1];
        used = used && is_fin(x0) && is_fin(x1);
        double ww = 1.0;
        if (a.conf) {
            ww = (a.conf + (vv * a.N + base))[i];
            ww = clamp_conf(ww);
            used = used && ww >= a.min_conf;
        }
        if (vv == v) {
            x[0] = x0;
            x[1] = x1;
            w = ww;
        }
    }
    return used;
}

// cyclic Jacobi of the symmetric n x n M (LDS, row stride n) to convergence, eigenvectors into the columns of Q; lane k
// owns row k in the column phase and column k in the row phase.  Every thread of the workgroup must call it.
__device__ void jacobi_lds(double* M, double* Q, int n) {
    const int k = threadIdx.x;
    for (int i = k; i < n * n; i += blockDim.x) Q[i] = (i / n == i % n) ? 1.0 : 0.0;
    __syncthreads();
    for (int sweep = 0; sweep < kJacobiSweeps; ++sweep) {
        double off = 0.0, diag = 0.0;
        for (int a = 0; a < n; ++a) {
            diag += M[a * n + a] * M[a * n + a];
            for (int b = a + 1; b < n; ++b) off += M[a * n + b] * M[a * n + b];
        }
        if (!is_fin(off) || off <= 1e-40 * diag || off == 0.0) break;
        for (int p = 0; p < n - 1; ++p)
            for (int q = p + 1; q < n; ++q) {
                const double mpq = M[p * n + q], mpp = M[p * n + p], mqq = M[q * n + q];
                __syncthreads();
                if (mpq == 0.0) continue;
                const double theta = (mqq - mpp) / (2.0 * mpq);
                const double tn = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double cs = 1.0 / sqrt(tn * tn + 1.0), sn = tn * cs;
                if (k < n) {
                    const double mkp = M[k * n + p], mkq = M[k * n + q];
                    M[k * n + p] = cs * mkp - sn * mkq;
                    M[k * n + q] = sn * mkp + cs * mkq;
                    const double qkp = Q[k * n + p], qkq = Q[k * n + q];
                    Q[k * n + p] = cs * qkp - sn * qkq;
                    Q[k * n + q] = sn * qkp + cs * qkq;
                }
                __syncthreads();
                if (k < n) {
                    const double mpk = M[p * n + k], mqk = M[q * n + k];
                    M[p * n + k] = k == q ? 0.0 : cs * mpk - sn * mqk;
                    M[q * n + k] = k == p ? 0.0 : sn * mpk + cs * mqk;
                }
                __syncthreads();
            }
    }
    __syncthreads();
}

// rule 5's solve: x with (H + lam I) x = -g, LDL^T without pivoting; H packed by rows of the upper triangle.  Every loop
// is unrolled, so the arrays are indexed by constants and stay in registers.
__device__ inline void ldl_solve(const double* Hp, const double* g, double lam, double* x) {
    double L[6][6], D[6], y[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double s = Hp[packed(j, j)] + lam;
#pragma unroll
        for (int k = 0; k < j; ++k) s -= L[j][k] * L[j][k] * D[k];
        D[j] = s;
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double e = Hp[packed(i, j)];
#pragma unroll
            for (int k = 0; k < j; ++k) e -= L[i][k] * L[j][k] * D[k];
            L[i][j] = e / D[j];
        }
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double s = -g[i];
#pragma unroll
        for (int k = 0; k < i; ++k) s -= L[i][k] * y[k];
        y[i] = s;
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) y[i] = y[i] / D[i];
#pragma unroll
    for (int i = 5; i >= 0; --i) {
        double s = y[i];
#pragma unroll
        for (int k = i + 1; k < 6; ++k) s -= L[k][i] * x[k];
        x[i] = s;
    }
}

template <int kThreads>
__global__ __launch_bounds__(kThreads) void resect_kernel(ResectArgs a) {
    __shared__ double red[2][kMaxWaves][kRed];
    __shared__ double sM[144], sQ[144], sP[12];
    __shared__ State s;
    const int tid = threadIdx.x, nt = blockDim.x;
    const long g = blockIdx.x / a.V;
    const int v = blockIdx.x % a.V;
    const long base = g * a.gs;
    const int gs = (int)a.gs;
    const long p = blockIdx.x;                 // problem index of the [G, V] outputs
    double* err = a.err + v * a.N + base;
    const double nan = qnan();

    // ---- rule 1: the count, and the sums of rule 2 and of the centroid ----
    double X[3], x[2], w;
    {
        double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int i = tid; i < gs; i += nt)
            if (load_point(a, base, i, v, X, x, w)) {
                acc[0] += 1.0;
                acc[1] += x[0];
                acc[2] += x[1];
                acc[3] += X[0];
                acc[4] += X[1];
                acc[5] += X[2];
            }
        block_sum<6>(acc, red[0]);
    }
    const double n = total(red[0], 0);
    if (tid == 0) {
        s.failed = n < kMinPoints ? 1 : 0;
        s.evals = 0;
        s.success = 0;
        s.first = 1;
        s.c = s.c0 = nan;
        if (a.K) {
            const double* K = a.K + 9 * v;
            s.K[0] = K[0], s.K[1] = K[1], s.K[2] = K[2], s.K[3] = K[4], s.K[4] = K[5];
        } else {
            s.K[0] = s.K[3] = nan;
            s.K[1] = 0.0;
            s.K[2] = total(red[0], 1) / n;
            s.K[4] = total(red[0], 2) / n;
        }
    }
    __syncthreads();
    bool failed = n < kMinPoints;
    if (!failed) {
        // ---- rule 2: K from the keypoints' spread (population std, second pass) ----
        if (!a.K) {
            const double cx = s.K[2], cy = s.K[4];
            double acc[2] = {0.0, 0.0};
            for (int i = tid; i < gs; i += nt)
                if (load_point(a, base, i, v, X, x, w)) {
                    acc[0] += (x[0] - cx) * (x[0] - cx);
                    acc[1] += (x[1] - cy) * (x[1] - cy);
                }
            block_sum<2>(acc, red[1]);
            if (tid == 0) {
                const double sx = sqrt(total(red[1], 0) / n) + 1e-6, sy = sqrt(total(red[1], 1) / n) + 1e-6;
                s.K[0] = s.K[3] = 2.0 * fmax(sx, sy);
            }
            __syncthreads();
        }
        // ---- rule 3: the start ----
        if (a.R0) {
            if (tid < 9) s.R[tid] = a.R0[9 * p + tid];
            if (tid < 3) s.t[tid] = a.t0[3 * p + tid];
        } else {
            const double c[3] = {total(red[0], 3) / n, total(red[0], 4) / n, total(red[0], 5) / n};
            double acc[1] = {0.0};
            for (int i = tid; i < gs; i += nt)
                if (load_point(a, base, i, v, X, x, w)) {
                    const double d0 = X[0] - c[0], d1 = X[1] - c[1], d2 = X[2] - c[2];
                    acc[0] += sqrt(d0 * d0 + d1 * d1 + d2 * d2);
                }
            block_sum<1>(acc, red[0]);         // red[0]'s centroid sums were read above by every thread
            const double sc = sqrt(3.0) / (total(red[0], 0) / n);
            const double fx = s.K[0], sk = s.K[1], cx = s.K[2], fy = s.K[3], cy = s.K[4];
            // A^T A of the rows [Xh, 0, -u Xh], [0, Xh, -v Xh] = [[S0, 0, -S1], [0, S0, -S2], [-S1, -S2, S3]] with
            // Sk = sum wk Xh Xh^T, wk = 1, u, v, u^2 + v^2: four passes of ten sums
            for (int k = 0; k < 4; ++k) {
                double acc10[10] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
                for (int i = tid; i < gs; i += nt)
                    if (load_point(a, base, i, v, X, x, w)) {
                        const double yv = (x[1] - cy) / fy, yu = (x[0] - cx - sk * yv) / fx;
                        const double wk = k == 0 ? 1.0 : k == 1 ? yu : k == 2 ? yv : yu * yu + yv * yv;
                        const double Xh[4] = {sc * (X[0] - c[0]), sc * (X[1] - c[1]), sc * (X[2] - c[2]), 1.0};
                        int m = 0;
#pragma unroll
                        for (int i0 = 0; i0 < 4; ++i0)
#pragma unroll
                            for (int i1 = i0; i1 < 4; ++i1) acc10[m++] += wk * (Xh[i0] * Xh[i1]);
                    }
                block_sum<10>(acc10, red[(k + 1) & 1]);
                if (tid == 0) {
                    const double(*rd)[kRed] = red[(k + 1) & 1];
                    int m = 0;
                    for (int i0 = 0; i0 < 4; ++i0)
                        for (int i1 = i0; i1 < 4; ++i1) {
                            const double val = total(rd, m++);
                            if (k == 0) {
                                sM[i0 * 12 + i1] = sM[i1 * 12 + i0] = val;
                                sM[(4 + i0) * 12 + 4 + i1] = sM[(4 + i1) * 12 + 4 + i0] = val;
                                sM[i0 * 12 + 4 + i1] = sM[i1 * 12 + 4 + i0] = 0.0;
                                sM[(4 + i0) * 12 + i1] = sM[(4 + i1) * 12 + i0] = 0.0;
                            } else if (k == 3) {
                                sM[(8 + i0) * 12 + 8 + i1] = sM[(8 + i1) * 12 + 8 + i0] = val;
                            } else {
                                const int r0 = 4 * (k - 1);
                                sM[(r0 + i0) * 12 + 8 + i1] = sM[(r0 + i1) * 12 + 8 + i0] = -val;
                                sM[(8 + i1) * 12 + r0 + i0] = sM[(8 + i0) * 12 + r0 + i1] = -val;
                            }
                        }
                }
            }
            __syncthreads();
            jacobi_lds(sM, sQ, 12);
            if (tid == 0) {
                int best = 0;
                for (int k = 1; k < 12; ++k)
                    if (sM[k * 12 + k] < sM[best * 12 + best]) best = k;
                for (int k = 0; k < 12; ++k) sP[k] = sQ[k * 12 + best];
                const double* P = sP;              // row-major 3 x 4; M = its left 3 x 3
                const double det = P[0] * (P[5] * P[10] - P[6] * P[9]) - P[1] * (P[4] * P[10] - P[6] * P[8]) +
                                   P[2] * (P[4] * P[9] - P[5] * P[8]);
                if (det < 0)
                    for (int k = 0; k < 12; ++k) sP[k] = -sP[k];
                for (int i0 = 0; i0 < 3; ++i0)         // M^T M
                    for (int i1 = 0; i1 < 3; ++i1)
                        sM[i0 * 3 + i1] = P[i0] * P[i1] + P[4 + i0] * P[4 + i1] + P[8 + i0] * P[8 + i1];
            }
            __syncthreads();
            jacobi_lds(sM, sQ, 3);
            if (tid == 0) {
                // R = M W diag(1 / sigma) W^T = U V^T of M = U S V^T; t = p4 3 / trace S, de-normalised
                double sig[3], MW[9];
#pragma unroll
                for (int k = 0; k < 3; ++k) sig[k] = sqrt(fmax(sM[k * 3 + k], 0.0));
#pragma unroll
                for (int i0 = 0; i0 < 3; ++i0)
#pragma unroll
                    for (int k = 0; k < 3; ++k)
                        MW[i0 * 3 + k] = (sP[4 * i0] * sQ[k] + sP[4 * i0 + 1] * sQ[3 + k] + sP[4 * i0 + 2] * sQ[6 + k]) * (1.0 / sig[k]);
#pragma unroll
                for (int i0 = 0; i0 < 3; ++i0)
#pragma unroll
                    for (int i1 = 0; i1 < 3; ++i1)
                        s.R[i0 * 3 + i1] = MW[i0 * 3] * sQ[i1 * 3] + MW[i0 * 3 + 1] * sQ[i1 * 3 + 1] + MW[i0 * 3 + 2] * sQ[i1 * 3 + 2];
                const double tr = sig[0] + sig[1] + sig[2];
                for (int k = 0; k < 3; ++k)
                    s.t[k] = (sP[4 * k + 3] * 3.0 / tr) / sc - (s.R[3 * k] * c[0] + s.R[3 * k + 1] * c[1] + s.R[3 * k + 2] * c[2]);
            }
        }
        __syncthreads();

        // ---- rules 4 and 5: Levenberg-Marquardt; thread 0 decides between the passes ----
        int phase = LINEARISE, buf = 0;
        while (phase != STOP) {
            if (phase == LINEARISE) {
                double acc[kRed];
#pragma unroll
                for (int k = 0; k < kRed; ++k) acc[k] = 0.0;
                for (int i = tid; i < gs; i += nt)
                    if (load_point(a, base, i, v, X, x, w)) {
                        Proj pr;
                        residual(s, X, x, w, pr);
                        // the x component, then the y component: J = [q x a, a] with a = d r / d Xc
#pragma unroll
                        for (int comp = 0; comp < 2; ++comp) {
                            double J[6];
                            if (comp == 0) {
                                J[3] = w * (s.K[0] / pr.z), J[4] = w * (s.K[1] / pr.z), J[5] = w * (-pr.pu / pr.z);
                            } else {
                                J[3] = 0.0, J[4] = w * (s.K[3] / pr.z), J[5] = w * (-(s.K[3] * pr.v) / pr.z);
                            }
                            cross3(pr.q, J + 3, J);
                            const double r = pr.r[comp];
                            // refine.hip's rho1_of, inline (a second copy, kept for the same reason as load_point)
                            double rho1 = 1.0;
                            if (a.soft) {
                                const double sq = sqrt(1.0 + (r / a.f_scale) * (r / a.f_scale));
                                rho1 = 1.0 / sq;
                                acc[27] += 2.0 * (sq - 1.0);
                            } else {
                                acc[27] += r * r;
                            }
                            int m = 0;
#pragma unroll
                            for (int i0 = 0; i0 < 6; ++i0)
#pragma unroll
                                for (int i1 = i0; i1 < 6; ++i1) acc[m++] += rho1 * (J[i0] * J[i1]);
#pragma unroll
                            for (int k = 0; k < 6; ++k) acc[21 + k] += rho1 * (J[k] * r);
                        }
                    }
                block_sum<kRed>(acc, red[buf]);
            } else {
                // the change of the cost under the step, formed from the step itself
                double acc[1] = {0.0};
                const double f2 = a.f_scale * a.f_scale;
                for (int i = tid; i < gs; i += nt)
                    if (load_point(a, base, i, v, X, x, w)) {
                        Proj pr;
                        residual(s, X, x, w, pr);
                        double c1[3], c2[3];
                        cross3(s.d, pr.q, c1);
                        cross3(s.d, c1, c2);
                        const double dX = s.A * c1[0] + s.B * c2[0] + s.d[3], dY = s.A * c1[1] + s.B * c2[1] + s.d[4],
                                     dZ = s.A * c1[2] + s.B * c2[2] + s.d[5];
                        const double z1 = pr.z + dZ;
                        const double du = (dX - pr.u * dZ) / z1, dv = (dY - pr.v * dZ) / z1;
                        const double drx = w * (s.K[0] * du + s.K[1] * dv), dry = w * (s.K[3] * dv);
                        // refine.hip's summand_change for both components, inline (a second copy, as above); the two
                        // summands are added to each other first, then to acc[0]
                        const double ex = drx * (2.0 * pr.r[0] + drx), ey = dry * (2.0 * pr.r[1] + dry);
                        if (a.soft) {
                            const double zx = (pr.r[0] / a.f_scale) * (pr.r[0] / a.f_scale), zy = (pr.r[1] / a.f_scale) * (pr.r[1] / a.f_scale);
                            const double dzx = ex / f2, dzy = ey / f2;
                            acc[0] += 2.0 * dzx / (sqrt(1.0 + (zx + dzx)) + sqrt(1.0 + zx)) + 2.0 * dzy / (sqrt(1.0 + (zy + dzy)) + sqrt(1.0 + zy));
                        } else {
                            acc[0] += ex + ey;
                        }
                    }
                block_sum<1>(acc, red[buf]);
            }
            if (tid == 0) {
                const double(*rd)[kRed] = red[buf];
                const double half = a.soft ? 0.5 * (a.f_scale * a.f_scale) : 0.5;
                int next = TRIAL;
                if (phase == LINEARISE) {
                    for (int k = 0; k < 21; ++k) s.H[k] = total(rd, k);
                    for (int k = 0; k < 6; ++k) s.g[k] = total(rd, 21 + k);
                    s.c = half * total(rd, 27);
                    bool ok = is_fin(s.c);
                    if (s.first) {
                        for (int k = 0; k < 9; ++k) ok = ok && is_fin(s.R[k]);
                        for (int k = 0; k < 3; ++k) ok = ok && is_fin(s.t[k]);
                        s.first = 0;
                        s.c0 = s.c;
                        s.evals = 1;
                        double hm = s.H[0];
                        for (int i0 = 1, m = 6; i0 < 6; m += 6 - i0, ++i0) hm = fmax(hm, s.H[m]);
                        s.lam = 1e-3 * hm;
                        if (!ok) {
                            s.failed = 1;
                            next = STOP;
                        }
                    } else if (!ok) {
                        next = STOP;
                    } else {
                        s.lam = s.lam / 10.0;
                        const double dn = sqrt(s.d[0] * s.d[0] + s.d[1] * s.d[1] + s.d[2] * s.d[2] + s.d[3] * s.d[3] + s.d[4] * s.d[4] + s.d[5] * s.d[5]);
                        const double tn = sqrt(s.t[0] * s.t[0] + s.t[1] * s.t[1] + s.t[2] * s.t[2]);
                        if (dn <= 1e-14 * (1.0 + tn)) {
                            s.success = 1;
                            next = STOP;
                        }
                    }
                } else {
                    const double dc = half * total(rd, 0);
                    if (is_fin(dc) && dc <= 1e-14 * s.c) {        // c + dc <= c (1 + 1e-14)
                        Rot r;
                        double R1[9];
                        rodrigues(s.d, r);
                        rotate(r, s.R, R1);
#pragma unroll
                        for (int k = 0; k < 9; ++k) s.R[k] = R1[k];
                        for (int k = 0; k < 3; ++k) s.t[k] = s.t[k] + s.d[3 + k];
                        next = LINEARISE;
                    } else {
                        s.lam = 10.0 * s.lam;
                        if (!(s.lam < 1e30)) {
                            s.success = 1;
                            next = STOP;
                        }
                    }
                }
                if (next == TRIAL) {
                    if (s.evals >= a.max_evals) {
                        next = STOP;
                    } else {
                        double d[6];
                        ldl_solve(s.H, s.g, s.lam, d);
#pragma unroll
                        for (int k = 0; k < 6; ++k) s.d[k] = d[k];
                        Rot r;
                        rodrigues(s.d, r);
                        s.A = r.A;
                        s.B = r.B;
                        s.evals = s.evals + 1;
                    }
                }
                s.next = next;
            }
            __syncthreads();
            phase = s.next;
            buf ^= 1;
        }
        failed = s.failed != 0;
    }

    // ---- rule 6: the final errors and the problem's record ----
    double acc[2] = {0.0, 0.0}, emax = 0.0;
    for (int i = tid; i < gs; i += nt) {
        double e = nan;
        if (load_point(a, base, i, v, X, x, w) && !failed) {
            Proj pr;
            residual(s, X, x, w, pr);
            const double dx = (pr.pu + s.K[2]) - x[0], dy = (s.K[3] * pr.v + s.K[4]) - x[1];
            e = sqrt(dx * dx + dy * dy);
            acc[0] += e;
            acc[1] += e * e;
            emax = max_nan(emax, e);
        }
        err[i] = e;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) emax = max_nan(emax, __shfl_down(emax, o, 64));
    // reduce.h's block_max by hand, in red's spare column: block_max needs an LDS array of its own and one more barrier
    __syncthreads();                           // the controller's last reads of red are done
    if ((tid & 63) == 0) red[0][tid >> 6][2] = emax;
    block_sum<2>(acc, red[0]);
    if (tid == 0) {
        for (int w0 = 1; w0 < (nt >> 6); ++w0) emax = max_nan(emax, red[0][w0][2]);
        for (int k = 0; k < 9; ++k) a.R[9 * p + k] = failed ? nan : s.R[k];
        for (int k = 0; k < 3; ++k) a.t[3 * p + k] = failed ? nan : s.t[k];
        double* K = a.K_out + 9 * p;
        K[0] = s.K[0], K[1] = s.K[1], K[2] = s.K[2], K[3] = 0.0, K[4] = s.K[3], K[5] = s.K[4], K[6] = 0.0, K[7] = 0.0, K[8] = 1.0;
        if (!a.K && n < kMinPoints)
            for (int k = 0; k < 9; ++k) K[k] = nan;
        a.cost0[p] = failed ? nan : s.c0;
        a.cost[p] = failed ? nan : s.c;
        a.n_evals[p] = failed ? 0 : s.evals;
        a.n_used[p] = (int32_t)n;
        a.success[p] = failed ? 0 : s.success;
        a.stats[3 * p] = failed ? nan : total(red[0], 0) / n;
        a.stats[3 * p + 1] = failed ? nan : sqrt(total(red[0], 1) / n);
        a.stats[3 * p + 2] = failed ? nan : emax;
    }
}

// R_rel = R_v R_0^T, t_rel = t_v - R_rel t_0 (slove_rt_from_3d.py:252-254), one thread per (group, view)
__global__ void relative_pose_kernel(const double* R, const double* t, long total_gv, int V, double* R_rel, double* t_rel) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total_gv) return;
    const long g0 = i / V * V;
    const double *Rv = R + 9 * i, *R0 = R + 9 * g0, *tv = t + 3 * i, *t0 = t + 3 * g0;
    double Rr[9];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) Rr[3 * a + b] = Rv[3 * a] * R0[3 * b] + Rv[3 * a + 1] * R0[3 * b + 1] + Rv[3 * a + 2] * R0[3 * b + 2];
#pragma unroll
    for (int k = 0; k < 9; ++k) R_rel[9 * i + k] = Rr[k];
#pragma unroll
    for (int a = 0; a < 3; ++a) t_rel[3 * i + a] = tv[a] - (Rr[3 * a] * t0[0] + Rr[3 * a + 1] * t0[1] + Rr[3 * a + 2] * t0[2]);
}

}  // namespace
}  // namespace skimi

using namespace skimi;

extern "C" {

size_t skimi_resect_workspace_bytes(int64_t n_points, int32_t views, int64_t group_size) {
    (void)n_points, (void)views, (void)group_size;
    return 0;      // every problem's state lives in its workgroup's LDS
}

int skimi_resect_cameras(const double* X, const double* x2d, const double* conf, const double* K, const double* R0,
                         const double* t0, int64_t n_points, int32_t views, int64_t group_size, int32_t loss, double f_scale,
                         double min_conf, int32_t max_evals, double* R, double* t, double* K_out, double* cost0, double* cost,
                         int32_t* n_evals, int32_t* n_used, int32_t* success, double* err, double* stats, void* ws,
                         size_t ws_bytes, void* stream) {
    (void)ws, (void)ws_bytes;
    SKIMI_CHECK_ARG(X && x2d, "skimi_resect_cameras: NULL input");
    SKIMI_CHECK_ARG(R && t && K_out && cost0 && cost && n_evals && n_used && success && err && stats,
                    "skimi_resect_cameras: NULL output");
    SKIMI_CHECK_ARG((R0 == nullptr) == (t0 == nullptr), "skimi_resect_cameras: R0 and t0 go together");
    SKIMI_CHECK_ARG(views >= 1 && views <= kMaxViews, "skimi_resect_cameras: %d views outside 1..%d", views, kMaxViews);
    SKIMI_CHECK_ARG(n_points >= 1 && group_size >= 1 && group_size <= n_points && n_points % group_size == 0,
                    "skimi_resect_cameras: group_size = %lld does not divide n_points = %lld", (long long)group_size,
                    (long long)n_points);
    SKIMI_CHECK_ARG(group_size <= kMaxGroup, "skimi_resect_cameras: group_size = %lld above %d (32-bit point offsets)",
                    (long long)group_size, kMaxGroup);
    const int64_t problems = n_points / group_size * views;
    SKIMI_CHECK_ARG(problems <= 0x7fffffffLL && n_points <= (1LL << 40), "skimi_resect_cameras: %lld problems or %lld points are too many",
                    (long long)problems, (long long)n_points);
    SKIMI_CHECK_ARG(loss == SKIMI_RESECT_LINEAR || loss == SKIMI_RESECT_SOFT_L1, "skimi_resect_cameras: unknown loss %d", loss);
    SKIMI_CHECK_ARG(f_scale > 0.0 && f_scale <= 1.79769313486231570815e308, "skimi_resect_cameras: f_scale = %g is not a positive number", f_scale);
    SKIMI_CHECK_ARG(min_conf == min_conf, "skimi_resect_cameras: min_conf is NaN");
    SKIMI_CHECK_ARG(max_evals >= 1, "skimi_resect_cameras: max_evals = %d < 1", max_evals);
    ResectArgs a{};
    a.X = X, a.x2d = x2d, a.conf = conf, a.K = K, a.R0 = R0, a.t0 = t0;
    a.R = R, a.t = t, a.K_out = K_out, a.cost0 = cost0, a.cost = cost, a.err = err, a.stats = stats;
    a.n_evals = n_evals, a.n_used = n_used, a.success = success;
    a.N = n_points, a.gs = group_size, a.V = views, a.soft = loss == SKIMI_RESECT_SOFT_L1, a.max_evals = max_evals;
    a.f_scale = f_scale, a.min_conf = min_conf;
    hipStream_t st = (hipStream_t)stream;
    if (group_size <= 64) {
        hipLaunchKernelGGL(resect_kernel<64>, dim3((unsigned)problems), dim3(64), 0, st, a);
    } else {
        const int threads = (int)(group_size >= 1024 ? 1024 : (group_size + 63) / 64 * 64);
        hipLaunchKernelGGL(resect_kernel<1024>, dim3((unsigned)problems), dim3(threads), 0, st, a);
    }
    SKIMI_LAUNCH_CHECK();
    return SKIMI_OK;
}

int skimi_relative_pose(const double* R, const double* t, int64_t groups, int32_t views, double* R_rel, double* t_rel,
                        void* stream) {
    SKIMI_CHECK_ARG(R && t && R_rel && t_rel, "skimi_relative_pose: NULL input or output");
    SKIMI_CHECK_ARG(groups >= 1 && views >= 1 && views <= kMaxViews && groups * views <= 0x7fffffffLL,
                    "skimi_relative_pose: groups = %lld, views = %d outside groups >= 1, 1 <= views <= %d", (long long)groups, views,
                    kMaxViews);
    const long n = groups * views;
    hipLaunchKernelGGL(relative_pose_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, R, t, n, views, R_rel,
                       t_rel);
    SKIMI_LAUNCH_CHECK();
    return SKIMI_OK;
}

}  // extern "C"
