// Bundle adjustment of one clip's cameras and joints (the clip-level refinement that vggt/multi_view_process.py:321-353
// defines but never runs; run_local_ba, :553-564, exists nowhere in the reference).  Loss = the five terms of
// bundle_adjustment/loss.py (reprojection, camera smoothness, baseline, bone length, pose temporal), minimised by Adam.
//
// One launch runs every iteration of every requested problem (mode): one workgroup per problem, no host round trip,
// no cross-workgroup traffic.  Per iteration (3 workgroup barriers):
//   P1  per (t,c): R = Exp(w) R0 (mode full), camera centre Cc = -R^T t                         -> scratch R, Cc
//   P2  per (t,c,j): projection, conf*residual^2, dLoss/dXcam                                    -> scratch g[t,c,j]
//       per t: baseline, the 12 bone lengths, the two temporal sums; one tree reduction of 16 values
//   P3  per (t,c): dt = sum_j g - R dCc, dR = sum_j g X^T - t dCc^T -> dw; Adam on t and w in place
//       per (t,j): dX = sum_c R^T g + temporal + bone terms; Adam on X into the other X buffer
//       one tree reduction of the bone and baseline loss values -> history row
// Every sum runs in a fixed order (per thread in item order, then reduce.h's fixed shuffle/wave tree): results are bitwise
// reproducible, and do not depend on where the state lives.  The state (parameters, Adam moments) and the per-iteration
// scratch live in LDS when they fit, else in the caller's workspace.  Rules: DESIGN §2 "BA".
#include <math.h>

#include "common.h"
#include "reduce.h"
#include "rodrigues.h"

namespace skimi {
namespace {

constexpr int kThreads = 512;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxC = 8, kMaxJ = 32, kMaxProblems = 8;
constexpr long kMaxT = 1L << 20;
constexpr int kBones = 12;
constexpr int kRed = 4 + kBones;                    // P2 sums: reprojection, smoothness, temporal, baseline, 12 bones
constexpr int kLdsDynMax = 160 * 1024 - 4096;       // 160 KiB per CU, less the static arrays below
constexpr double kB1 = 0.9, kB2 = 0.999, kEps = 1e-8;
constexpr double kZmin = 1e-6;

// bundle_adjustment/loss.py:118-131 (COCO-17 indices)
__constant__ int kBone[kBones][2] = {{11, 13}, {13, 15}, {12, 14}, {14, 16}, {5, 7}, {7, 9},
                                     {6, 8},   {8, 10},  {5, 6},   {11, 12}, {5, 11}, {6, 12}};

enum Mode { POSE_ONLY = 0, POSE_CAM_T = 1, FULL = 2 };

struct BaArgs {
    const double *K, *R0, *t0, *X0, *x2d, *conf;
    double *R_out, *t_out, *X_out, *hist;
    double* ws;
    long per;                                        // doubles per problem (state + scratch)
    int T, C, J, iters;
    double lr, w[5];                                 // reprojection, smoothness, baseline, bone length, temporal
    int modes[kMaxProblems];
};

// doubles of one problem: X (2 buffers), mX, vX | t, mt, vt | w, mw, vw | R | Cc | g
__host__ __device__ inline long per_problem(long T, long C, long J) {
    const long nX = T * J * 3, nC = T * C * 3;
    return (4 * nX + 10 * nC + nC * J + 31) / 32 * 32;   // 256-B aligned problems
}

// <M, [e_k]x> for k = 0, 1, 2
__device__ inline void skew_dot(const double* M, double* s) {
    s[0] = M[7] - M[5];
    s[1] = M[2] - M[6];
    s[2] = M[3] - M[1];
}

__device__ inline void adam(double& p, double& m, double& v, double g, double step_size, double bc2_sqrt) {
    m = kB1 * m + (1.0 - kB1) * g;
    v = kB2 * v + (1.0 - kB2) * (g * g);
    p = p - step_size * (m / (sqrt(v) / bc2_sqrt + kEps));
}

template <bool kLds>
__global__ __launch_bounds__(kThreads) void ba_kernel(BaArgs a) {
    extern __shared__ double dyn[];
    __shared__ double red[2][kWaves][kRed];
    __shared__ double sK[kMaxC * 9];
    const int p = blockIdx.x, mode = a.modes[p], tid = threadIdx.x;
    const int T = a.T, C = a.C, J = a.J;
    const int nX = T * J * 3, nC = T * C * 3, TC = T * C, TJ = T * J, TCJ = T * C * J;
    double* base = kLds ? dyn : a.ws + (long)p * a.per;
    double* X0b = base;
    double* X1b = base + nX;
    double* mX = base + 2 * nX;
    double* vX = mX + nX;
    double* tt = vX + nX;
    double* mt = tt + nC;
    double* vt = mt + nC;
    double* ww = vt + nC;
    double* mw = ww + nC;
    double* vw = mw + nC;
    double* sR = vw + nC;
    double* sCc = sR + 3 * nC;
    double* sg = sCc + nC;

    for (int i = tid; i < nX; i += kThreads) {
        X0b[i] = a.X0[i];
        mX[i] = 0.0;
        vX[i] = 0.0;
    }
    for (int i = tid; i < nC; i += kThreads) {
        tt[i] = a.t0[i];
        mt[i] = vt[i] = ww[i] = mw[i] = vw[i] = 0.0;
    }
    for (int i = tid; i < 3 * nC; i += kThreads) sR[i] = a.R0[i];
    for (int i = tid; i < C * 9; i += kThreads) sK[i] = a.K[i];
    double cs[1] = {0.0};
    for (int i = tid; i < TCJ; i += kThreads) cs[0] += a.conf[i];
    block_sum<1>(cs, red[1]);          // its barrier also publishes the initial state
    const double S = total<kWaves>(red[1], 0) + 1e-6;     // loss.py:94

    int nb = 0;                        // bones with both indices < J (loss.py:137-139)
    for (int b = 0; b < kBones; ++b) nb += (kBone[b][0] < J && kBone[b][1] < J) ? 1 : 0;
    const double w_rep = a.w[0], w_smooth = a.w[1], w_base = a.w[2], w_bone = a.w[3], w_temp = a.w[4];
    const double Ns = (double)(T - 1) * C * 3, Np = (double)(T - 1) * J * 3, Nb = (double)T * nb;
    const double c_rep = 2.0 * w_rep / S, c_smooth = 2.0 * w_smooth / Ns, c_temp = 2.0 * w_temp / Np;
    const double c_base = 2.0 * w_base / T, c_bone = 2.0 * w_bone / Nb;
    double* hist = a.hist ? a.hist + (long)p * a.iters * 6 : nullptr;

    for (int it = 0; it < a.iters; ++it) {
        const double* Xc = (it & 1) ? X1b : X0b;
        double* Xn = (it & 1) ? X0b : X1b;
        // ---- P1: rotations and camera centres ----
        for (int i = tid; i < TC; i += kThreads) {
            double R[9];
            if (mode == FULL) {
                Rot r;
                rodrigues(ww + 3 * i, r);
                rotate(r, a.R0 + 9 * i, R);
#pragma unroll
                for (int k = 0; k < 9; ++k) sR[9 * i + k] = R[k];
            } else {
#pragma unroll
                for (int k = 0; k < 9; ++k) R[k] = sR[9 * i + k];
            }
            const double* tv = tt + 3 * i;
#pragma unroll
            for (int k = 0; k < 3; ++k) sCc[3 * i + k] = -(R[k] * tv[0] + R[3 + k] * tv[1] + R[6 + k] * tv[2]);
        }
        __syncthreads();
        // ---- P2: reprojection partials and the sums the gradients need ----
        double acc[kRed];
#pragma unroll
        for (int k = 0; k < kRed; ++k) acc[k] = 0.0;
        for (int i = tid; i < TCJ; i += kThreads) {
            const int tc = i / J, j = i - tc * J, t = tc / C, c = tc - t * C;
            const double* R = sR + 9 * tc;
            const double* X = Xc + 3 * (t * J + j);
            const double* tv = tt + 3 * tc;
            const double* Kc = sK + 9 * c;
            double xc[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) xc[k] = R[3 * k] * X[0] + R[3 * k + 1] * X[1] + R[3 * k + 2] * X[2] + tv[k];
            const bool clamped = xc[2] < kZmin;     // clamp(min=1e-6): no gradient to Z below the bound
            const double z = clamped ? kZmin : xc[2];
            const double u = xc[0] / z, v = xc[1] / z;
            const double dx = (Kc[0] * u + Kc[1] * v + Kc[2]) - a.x2d[2 * i];
            const double dy = (Kc[3] * u + Kc[4] * v + Kc[5]) - a.x2d[2 * i + 1];
            const double cf = a.conf[i];
            acc[0] += cf * (dx * dx + dy * dy);
            const double gpx = c_rep * cf * dx, gpy = c_rep * cf * dy;
            const double gu = gpx * Kc[0] + gpy * Kc[3], gv = gpx * Kc[1] + gpy * Kc[4];
            double* g = sg + 3 * i;
            g[0] = gu / z;
            g[1] = gv / z;
            g[2] = clamped ? 0.0 : -(gu * u + gv * v) / z;
        }
        for (int t = tid; t < T; t += kThreads) {
            if (C >= 2) {
                const double* c0 = sCc + 3 * (t * C);
                const double d0 = c0[0] - c0[3], d1 = c0[1] - c0[4], d2 = c0[2] - c0[5];
                acc[3] += sqrt(d0 * d0 + d1 * d1 + d2 * d2);
            }
            const double* Xt = Xc + 3 * t * J;
#pragma unroll
            for (int b = 0; b < kBones; ++b) {
                const int i0 = kBone[b][0], i1 = kBone[b][1];
                if (i0 < J && i1 < J) {
                    const double s0 = Xt[3 * i0] - Xt[3 * i1], s1 = Xt[3 * i0 + 1] - Xt[3 * i1 + 1], s2 = Xt[3 * i0 + 2] - Xt[3 * i1 + 2];
                    acc[4 + b] += sqrt(s0 * s0 + s1 * s1 + s2 * s2);
                }
            }
            if (t + 1 < T) {
                const double* cA = sCc + 3 * (t * C);
                for (int k = 0; k < 3 * C; ++k) {
                    const double d = cA[3 * C + k] - cA[k];
                    acc[1] += d * d;
                }
                for (int k = 0; k < 3 * J; ++k) {
                    const double d = Xt[3 * J + k] - Xt[k];
                    acc[2] += d * d;
                }
            }
        }
        block_sum<kRed>(acc, red[0]);
        const double bm = total<kWaves>(red[0], 3) / T;        // baseline mean, held constant (detach)
        // ---- P3: gradients and Adam ----
        const double bc1 = 1.0 - pow(kB1, (double)(it + 1)), bc2_sqrt = sqrt(1.0 - pow(kB2, (double)(it + 1)));
        const double step = a.lr / bc1;
        double acc2[2] = {0.0, 0.0};         // bone length loss sum, baseline loss sum
        for (int i = tid; i < TC; i += kThreads) {
            const int t = i / C, c = i - t * C;
            const double* Cc = sCc + 3 * i;
            double dC[3] = {0.0, 0.0, 0.0};
            if (C >= 2 && c < 2) {
                const double* c0 = sCc + 3 * (t * C);
                const double d[3] = {c0[0] - c0[3], c0[1] - c0[4], c0[2] - c0[5]};
                const double b = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
                if (c == 0) acc2[1] += (b - bm) * (b - bm);
                if (b > 0.0) {               // torch.norm backward: 0 at a zero-length baseline
                    const double sc = (c_base * (b - bm)) / b;
#pragma unroll
                    for (int k = 0; k < 3; ++k) dC[k] = c == 0 ? d[k] * sc : -(d[k] * sc);
                }
            }
            if (mode == POSE_ONLY) continue;
            if (T > 1) {
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const double back = t > 0 ? Cc[k] - Cc[k - 3 * C] : 0.0;
                    const double fwd = t + 1 < T ? Cc[k + 3 * C] - Cc[k] : 0.0;
                    dC[k] += c_smooth * (back - fwd);
                }
            }
            const double* R = sR + 9 * i;
            double* tv = tt + 3 * i;
            double gs[3] = {0.0, 0.0, 0.0}, GX[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) GX[k] = 0.0;
            for (int j = 0; j < J; ++j) {
                const double* g = sg + 3 * (i * J + j);
                const double* X = Xc + 3 * (t * J + j);
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    gs[r] += g[r];
#pragma unroll
                    for (int q = 0; q < 3; ++q) GX[3 * r + q] += g[r] * X[q];
                }
            }
            double dt[3];
#pragma unroll
            for (int r = 0; r < 3; ++r) dt[r] = gs[r] - (R[3 * r] * dC[0] + R[3 * r + 1] * dC[1] + R[3 * r + 2] * dC[2]);
            if (mode == FULL) {
                double G[9], Gp[9];          // dLoss/dR, then dLoss/dE = G R0^T
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int q = 0; q < 3; ++q) G[3 * r + q] = GX[3 * r + q] - tv[r] * dC[q];
                const double* R0 = a.R0 + 9 * i;
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int q = 0; q < 3; ++q) Gp[3 * r + q] = G[3 * r] * R0[3 * q] + G[3 * r + 1] * R0[3 * q + 1] + G[3 * r + 2] * R0[3 * q + 2];
                double* wv = ww + 3 * i;
                Rot rt;
                rodrigues(wv, rt);
                double H[9];                 // G' K^T + K^T G'
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int q = 0; q < 3; ++q)
                        H[3 * r + q] = (Gp[3 * r] * rt.Kx[3 * q] + Gp[3 * r + 1] * rt.Kx[3 * q + 1] + Gp[3 * r + 2] * rt.Kx[3 * q + 2]) +
                                       (rt.Kx[r] * Gp[q] + rt.Kx[3 + r] * Gp[3 + q] + rt.Kx[6 + r] * Gp[6 + q]);
                double gK = 0.0, gK2 = 0.0;
#pragma unroll
                for (int k = 0; k < 9; ++k) {
                    gK += Gp[k] * rt.Kx[k];
                    gK2 += Gp[k] * rt.K2[k];
                }
                double sG[3], sH[3];
                skew_dot(Gp, sG);
                skew_dot(H, sH);
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const double dw = rt.a1 * wv[k] * gK + rt.A * sG[k] + rt.b1 * wv[k] * gK2 + rt.B * sH[k];
                    adam(wv[k], mw[3 * i + k], vw[3 * i + k], dw, step, bc2_sqrt);
                }
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) adam(tv[k], mt[3 * i + k], vt[3 * i + k], dt[k], step, bc2_sqrt);
        }
        for (int i = tid; i < TJ; i += kThreads) {
            const int t = i / J, j = i - t * J;
            const double* X = Xc + 3 * i;
            double dX[3] = {0.0, 0.0, 0.0};
            for (int c = 0; c < C; ++c) {
                const double* R = sR + 9 * (t * C + c);
                const double* g = sg + 3 * ((t * C + c) * J + j);
#pragma unroll
                for (int k = 0; k < 3; ++k) dX[k] += R[k] * g[0] + R[3 + k] * g[1] + R[6 + k] * g[2];
            }
            if (T > 1) {
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const double back = t > 0 ? X[k] - X[k - 3 * J] : 0.0;
                    const double fwd = t + 1 < T ? X[k + 3 * J] - X[k] : 0.0;
                    dX[k] += c_temp * (back - fwd);
                }
            }
            const double* Xt = Xc + 3 * t * J;
#pragma unroll
            for (int b = 0; b < kBones; ++b) {
                const int i0 = kBone[b][0], i1 = kBone[b][1];
                if (i0 >= J || i1 >= J || (j != i0 && j != i1)) continue;
                const double s[3] = {Xt[3 * i0] - Xt[3 * i1], Xt[3 * i0 + 1] - Xt[3 * i1 + 1], Xt[3 * i0 + 2] - Xt[3 * i1 + 2]};
                const double L = sqrt(s[0] * s[0] + s[1] * s[1] + s[2] * s[2]);
                const double dL = L - total<kWaves>(red[0], 4 + b) / T;    // reference length: mean over T, held constant (detach)
                if (j == i0) acc2[0] += dL * dL;
                if (L > 0.0) {               // torch.norm backward: 0 at a zero-length bone
                    const double sc = (c_bone * dL) / L;
#pragma unroll
                    for (int k = 0; k < 3; ++k) dX[k] += j == i0 ? s[k] * sc : -(s[k] * sc);
                }
            }
            double* xn = Xn + 3 * i;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                double pk = X[k];
                adam(pk, mX[3 * i + k], vX[3 * i + k], dX[k], step, bc2_sqrt);
                xn[k] = pk;
            }
        }
        block_sum<2>(acc2, red[1]);
        if (tid == 0 && hist) {
            const double l_rep = w_rep * total<kWaves>(red[0], 0) / S;
            const double l_smooth = T > 1 ? w_smooth * (total<kWaves>(red[0], 1) / Ns) : 0.0;
            const double l_base = C >= 2 ? w_base * (total<kWaves>(red[1], 1) / T) : 0.0;
            const double l_bone = nb > 0 ? w_bone * (total<kWaves>(red[1], 0) / Nb) : 0.0;
            const double l_temp = T > 1 ? w_temp * (total<kWaves>(red[0], 2) / Np) : 0.0;
            double* h = hist + 6L * it;
            h[0] = l_rep + l_smooth + l_base + l_bone + l_temp;
            h[1] = l_rep;
            h[2] = l_smooth;
            h[3] = l_base;
            h[4] = l_bone;
            h[5] = l_temp;
        }
    }
    // ---- outputs: blocks the mode does not optimise are copied from the inputs ----
    const double* Xf = (a.iters & 1) ? X1b : X0b;
    double* Xo = a.X_out + (long)p * nX;
    double* to = a.t_out + (long)p * nC;
    double* Ro = a.R_out + (long)p * 3 * nC;
    for (int i = tid; i < nX; i += kThreads) Xo[i] = Xf[i];
    for (int i = tid; i < nC; i += kThreads) to[i] = mode == POSE_ONLY ? a.t0[i] : tt[i];
    for (int i = tid; i < TC; i += kThreads) {
        if (mode == FULL) {
            Rot r;
            rodrigues(ww + 3 * i, r);
            rotate(r, a.R0 + 9 * i, Ro + 9 * i);
        } else {
#pragma unroll
            for (int k = 0; k < 9; ++k) Ro[9 * i + k] = a.R0[9 * i + k];
        }
    }
}

}  // namespace
}  // namespace skimi

using namespace skimi;

extern "C" {

size_t skimi_ba_workspace_bytes(int64_t T, int32_t C, int32_t J, int32_t modes) {
    if (T < 1 || T > kMaxT || C < 1 || C > kMaxC || J < 1 || J > kMaxJ || modes < 1 || modes > kMaxProblems) return 0;
    return (size_t)per_problem(T, C, J) * sizeof(double) * (size_t)modes;
}

int skimi_bundle_adjust(const double* K, const double* R0, const double* t0, const double* X0, const double* x2d,
                        const double* conf, int64_t T, int32_t C, int32_t J, const int32_t* modes, int32_t n_modes,
                        int32_t num_iters, double lr, double w_reproj, double w_smooth, double w_baseline,
                        double w_bone_length, double w_pose_temporal, int32_t placement, double* R_out, double* t_out,
                        double* X_out, double* history_out, void* ws, size_t ws_bytes, void* stream) {
    SKIMI_CHECK_ARG(K && R0 && t0 && X0 && x2d && conf && modes && R_out && t_out && X_out,
                    "skimi_bundle_adjust: NULL input or output");
    SKIMI_CHECK_ARG(T >= 1 && T <= kMaxT && C >= 1 && C <= kMaxC && J >= 1 && J <= kMaxJ,
                    "skimi_bundle_adjust: T = %lld, C = %d, J = %d outside 1 <= T <= %ld, 1 <= C <= %d, 1 <= J <= %d",
                    (long long)T, C, J, kMaxT, kMaxC, kMaxJ);
    SKIMI_CHECK_ARG(n_modes >= 1 && n_modes <= kMaxProblems, "skimi_bundle_adjust: %d problems (1..%d)", n_modes, kMaxProblems);
    SKIMI_CHECK_ARG(num_iters >= 0, "skimi_bundle_adjust: num_iters = %d < 0", num_iters);
    SKIMI_CHECK_ARG(placement >= SKIMI_BA_AUTO && placement <= SKIMI_BA_WORKSPACE, "skimi_bundle_adjust: unknown placement %d",
                    placement);
    BaArgs a{};
    for (int p = 0; p < n_modes; ++p) {
        SKIMI_CHECK_ARG(modes[p] >= SKIMI_BA_POSE_ONLY && modes[p] <= SKIMI_BA_FULL, "skimi_bundle_adjust: unknown mode %d",
                        modes[p]);
        a.modes[p] = modes[p];
    }
    a.per = per_problem(T, C, J);
    const size_t need = (size_t)a.per * sizeof(double) * (size_t)n_modes;
    const bool fits = (size_t)a.per * sizeof(double) <= (size_t)kLdsDynMax;
    SKIMI_CHECK_ARG(placement != SKIMI_BA_LDS || fits, "skimi_bundle_adjust: the state of %zu bytes does not fit in LDS (%d)",
                    (size_t)a.per * sizeof(double), kLdsDynMax);
    const bool lds = placement == SKIMI_BA_LDS || (placement == SKIMI_BA_AUTO && fits);
    if (!lds && ws_bytes < need) {
        set_error("skimi_bundle_adjust: workspace of %zu bytes < skimi_ba_workspace_bytes = %zu", ws_bytes, need);
        return SKIMI_ERR_WORKSPACE;
    }
    SKIMI_CHECK_ARG(lds || ws, "skimi_bundle_adjust: NULL workspace");
    a.K = K;
    a.R0 = R0;
    a.t0 = t0;
    a.X0 = X0;
    a.x2d = x2d;
    a.conf = conf;
    a.R_out = R_out;
    a.t_out = t_out;
    a.X_out = X_out;
    a.hist = history_out;
    a.ws = (double*)ws;
    a.T = (int)T;
    a.C = C;
    a.J = J;
    a.iters = num_iters;
    a.lr = lr;
    a.w[0] = w_reproj;
    a.w[1] = w_smooth;
    a.w[2] = w_baseline;
    a.w[3] = w_bone_length;
    a.w[4] = w_pose_temporal;
    hipStream_t st = (hipStream_t)stream;
    if (lds) {
        const int bytes = (int)(a.per * sizeof(double));
        SKIMI_LDS_OPT_IN(ba_kernel<true>, kLdsDynMax, "ba_kernel");
        hipLaunchKernelGGL(ba_kernel<true>, dim3(n_modes), dim3(kThreads), bytes, st, a);
    } else {
        hipLaunchKernelGGL(ba_kernel<false>, dim3(n_modes), dim3(kThreads), 0, st, a);
    }
    SKIMI_LAUNCH_CHECK();
    return SKIMI_OK;
}

}  // extern "C"
