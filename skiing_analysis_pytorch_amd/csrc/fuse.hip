// The consumers of the gathered [T, J, 3] joints on the device: the VideoPose3D left/right fusion without extrinsics
// (fuse.fuse_pose_no_extrinsics_h36m), the two-view fusion with its confidences (the per-frame body of fuse/main_raw.py:
// align_right_to_left, weakpersp_reproj_confidence, crossview_consistency_confidence, fuse_frame_3d), the adaptive EMA
// (fuse.temporal_smooth_ema) and the NaN-aware Savitzky-Golay filter (fuse.smooth_skeleton); the fusion of every pair of a
// camera group (fuse/main_unity.py) through the two-view kernel's device functions, the EMA of a batch of clips, and the
// ground-truth-free joint quality (fuse/fuse.py:124-285).  The host functions of fuse.py are the restatement; rules: DESIGN
// §2 "Fusion + smoothing on the device", "Group fusion", "Joint quality".
//
// Fusion: one wave per frame (four frames per workgroup, no LDS, no barrier), lanes over joints (two joints per lane above
// 64).  Every sum is a per-lane sum over the lane's joints followed by a fixed xor-butterfly over the 64 lanes, so it
// depends on nothing but the frame's own data and every lane ends with the same bits: the 3 x 3 decomposition then runs
// uniformly across the wave (one lane's time, no broadcast).  The polar factors come from a one-sided (Hestenes) Jacobi
// SVD: the columns are rotated until they are orthogonal, which keeps the small singular value to relative accuracy where
// the eigen-decomposition of M^T M would square the condition number.
// Smoothing: one thread per joint (EMA) or per (joint, coordinate) series (Savitzky-Golay), sequential in t, the loads of
// eight steps issued together; neighbouring threads read neighbouring addresses.  All arithmetic is float64 and the file
// is compiled without FMA contraction, so a x + (1 - a) y is two products and a sum wherever it appears.
#include <math.h>

#include "common.h"
#include "fp64_util.h"
#include "reduce.h"
#include "svd3.h"

namespace skimi {
namespace {

constexpr int kH36mJoints = 17;
constexpr int kMaxJoints = 128;              // two joints per lane
constexpr int kMaxWin = 33;                  // Savitzky-Golay window: the ring of a series lives in LDS
constexpr int kBatch = 8;                    // time steps loaded together by the smoothers
constexpr unsigned kTorsoMask = (1u << 0) | (1u << 9) | (1u << 4) | (1u << 1) | (1u << 11) | (1u << 14);

// ---- VideoPose3D left/right fusion ---------------------------------------------------------------------------------
struct H36mArgs {
    const double *left, *right, *tau_j, *wL, *wR;
    double *fused, *R, *t, *s, *diag;
    int32_t* status;
    long T, wL_stride, wR_stride;
    double tau;
    int allow_scale, mirror;
};

// center_scale_h36m over the wave: pelvis (lane 0) to the origin, pelvis-neck (lane 9) distance 1 unless it is not > 1e-8
__device__ inline void center_scale(double* X) {
    double p[3], d[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        p[c] = __shfl(X[c], 0, 64);
        d[c] = __shfl(X[c], 9, 64) - p[c];
    }
    double s = norm3(d[0], d[1], d[2]);
    s = s > 1e-8 ? s : 1.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) X[c] = (X[c] - p[c]) / s;
}

__global__ __launch_bounds__(256) void fuse_h36m_kernel(H36mArgs a) {
    const int lane = threadIdx.x & 63;
    const long t = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= a.T) return;                      // the whole wave leaves: no barrier in this kernel
    const bool act = lane < kH36mJoints;
    const int j = act ? lane : 0;
    const double nan = qnan();
    double L[3], Rn[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        L[c] = a.left[(t * kH36mJoints + j) * 3 + c];
        Rn[c] = a.right[(t * kH36mJoints + j) * 3 + c];
    }
    if (a.mirror) {
        Rn[0] = -Rn[0];
        Rn[2] = -Rn[2];
    }
    center_scale(L);
    center_scale(Rn);
    // estimate_rigid_umeyama(X = left torso, Y = right torso) on the rows finite on both sides
    const bool tor = act && ((kTorsoMask >> lane) & 1u) && fin3(L) && fin3(Rn);
    const double n = wave_sum(tor ? 1.0 : 0.0);
    double* Ro = a.R + 9 * t;
    double* to = a.t + 3 * t;
    double* dg = a.diag + 4 * t;
    if (n < 3.0) {
        if (act)
            for (int c = 0; c < 3; ++c) a.fused[(t * kH36mJoints + j) * 3 + c] = nan;
        if (lane == 0) {
            for (int k = 0; k < 9; ++k) Ro[k] = nan;
            for (int k = 0; k < 3; ++k) to[k] = nan;
            for (int k = 0; k < 4; ++k) dg[k] = nan;
            a.s[t] = nan;
            a.status[t] = 0;
        }
        return;
    }
    double mx[3], my[3], Xc[3], Yc[3], Sg[9];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        mx[c] = wave_sum(tor ? L[c] : 0.0) / n;
        my[c] = wave_sum(tor ? Rn[c] : 0.0) / n;
        Xc[c] = L[c] - mx[c];
        Yc[c] = Rn[c] - my[c];
    }
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) Sg[3 * r + c] = wave_sum(tor ? Yc[r] * Xc[c] : 0.0) / n;
    const double vy = wave_sum(tor ? Yc[0] * Yc[0] + Yc[1] * Yc[1] + Yc[2] * Yc[2] : 0.0);
    double Rm[9], ssum;
    polar3(Sg, Rm, ssum);
    const double s = a.allow_scale ? ssum / (vy / n + 1e-12) : 1.0;
    double tv[3], Al[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        tv[r] = mx[r] - s * (Rm[3 * r] * my[0] + Rm[3 * r + 1] * my[1] + Rm[3 * r + 2] * my[2]);
        Al[r] = s * (Rm[3 * r] * Rn[0] + Rm[3 * r + 1] * Rn[1] + Rm[3 * r + 2] * Rn[2]) + tv[r];
    }
    // fuse_two
    const double tau = a.tau_j ? a.tau_j[j] : a.tau;
    const double wl = a.wL ? a.wL[t * a.wL_stride + j] : 1.0, wr = a.wR ? a.wR[t * a.wR_stride + j] : 1.0;
    const bool lok = fin3(L), rok = fin3(Al);
    double F[3];
    const bool far = norm3(L[0] - Al[0], L[1] - Al[1], L[2] - Al[2]) > tau;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double blend = (wl * L[c] + wr * Al[c]) / (wl + wr + 1e-9);
        const double pick = far ? (wl >= wr ? L[c] : Al[c]) : blend;
        F[c] = lok ? (rok ? pick : L[c]) : (rok ? Al[c] : nan);
    }
    center_scale(F);
    const double before = wave_sum(act ? norm3(L[0] - Rn[0], L[1] - Rn[1], L[2] - Rn[2]) : 0.0) / kH36mJoints;
    const double to_l = wave_sum(act ? norm3(F[0] - L[0], F[1] - L[1], F[2] - L[2]) : 0.0) / kH36mJoints;
    const double to_r = wave_sum(act ? norm3(F[0] - Rn[0], F[1] - Rn[1], F[2] - Rn[2]) : 0.0) / kH36mJoints;
    if (act)
        for (int c = 0; c < 3; ++c) a.fused[(t * kH36mJoints + j) * 3 + c] = F[c];
    if (lane == 0) {
        for (int k = 0; k < 9; ++k) Ro[k] = Rm[k];
        for (int k = 0; k < 3; ++k) to[k] = tv[k];
        dg[0] = before, dg[1] = to_l, dg[2] = to_r, dg[3] = before - 0.5 * (to_l + to_r);
        a.s[t] = s;
        a.status[t] = 1;
    }
}

// ---- two-view fusion with confidences ------------------------------------------------------------------------------
struct ViewsArgs {
    const double *Xl, *Xr, *Ul, *Ur;
    double *fused, *aligned, *q_l, *q_r, *conf_l, *conf_r, *conf_x, *err_l, *err_r, *dist;
    int32_t* fit_ok;
    long T;
    int J, key[5], torso, min_points;
    double sigma_px, sigma_3d;
};

// weakpersp_reproj_confidence of one view: u ~ s (X M) + t fitted on the rows finite in X and U -> conf, err per joint;
// false (conf 0, err NaN) for fewer than min_points rows or an energy under 1e-12, where the host raises
__device__ inline bool weakpersp(const double (*X)[3], const double (*U)[2], const bool* act, int min_points, double sigma,
                                 double* conf, double* err) {
    const double nan = qnan();
    bool used[2];
    double cnt = 0.0;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        used[k] = act[k] && fin3(X[k]) && is_fin(U[k][0]) && is_fin(U[k][1]);
        cnt += used[k] ? 1.0 : 0.0;
    }
    const double n = wave_sum(cnt);
    double mx[3], mu[2], A[9], energy = 0.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) mx[c] = wave_sum((used[0] ? X[0][c] : 0.0) + (used[1] ? X[1][c] : 0.0)) / n;
#pragma unroll
    for (int c = 0; c < 2; ++c) mu[c] = wave_sum((used[0] ? U[0][c] : 0.0) + (used[1] ? U[1][c] : 0.0)) / n;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 2; ++c)
            A[3 * r + c] = wave_sum((used[0] ? (X[0][r] - mx[r]) * (U[0][c] - mu[c]) : 0.0) +
                                (used[1] ? (X[1][r] - mx[r]) * (U[1][c] - mu[c]) : 0.0));
        A[3 * r + 2] = 0.0;
        energy += wave_sum((used[0] ? (X[0][r] - mx[r]) * (X[0][r] - mx[r]) : 0.0) + (used[1] ? (X[1][r] - mx[r]) * (X[1][r] - mx[r]) : 0.0));
    }
    const bool ok = n >= (double)min_points && !(energy < 1e-12) && n > 0.0;
    double M[9], ssum;
    polar3(A, M, ssum);                        // M[:, :2] = P[:, :2] Q^T
    const double s = ssum / energy;
    double tt[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) tt[c] = mu[c] - s * (mx[0] * M[c] + mx[1] * M[3 + c] + mx[2] * M[6 + c]);
    const double sg = fmax(sigma, 1e-12), var = sg * sg;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const double h0 = s * (X[k][0] * M[0] + X[k][1] * M[3] + X[k][2] * M[6]) + tt[0];
        const double h1 = s * (X[k][0] * M[1] + X[k][1] * M[4] + X[k][2] * M[7]) + tt[1];
        const bool fin = ok && act[k] && is_fin(U[k][0]) && is_fin(U[k][1]) && is_fin(h0) && is_fin(h1);
        const double d0 = h0 - U[k][0], d1 = h1 - U[k][1];
        const double e = fin ? sqrt(d0 * d0 + d1 * d1) : nan;
        err[k] = e;
        conf[k] = is_fin(e) ? exp(-(e * e) / (2.0 * var)) : 0.0;
    }
    return ok;
}

__device__ inline void unit3(double* v, double eps) {
    const double n = norm3(v[0], v[1], v[2]);
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = n < eps ? v[c] * 0.0 : v[c] / n;
}

// canonicalize_pose_3d: the frame's pose `F` ([J, 3] in memory, for the key joints) applied to the lane's rows X -> C;
// a missing key joint or a degenerate scale gives NaN rows
__device__ inline void canonicalize(const double* F, const int* key, int torso, const double (*X)[3], double (*C)[3]) {
    const double nan = qnan();
    double K[5][3];
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 5; ++i)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            K[i][c] = F[3 * key[i] + c];
            ok = ok && is_fin(K[i][c]);
        }
    double lh[3], rh[3], hips[3], sh[3], ex[3], ey[3], ez[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        lh[c] = K[1][c] - K[0][c];
        rh[c] = K[2][c] - K[0][c];
        hips[c] = 0.5 * (lh[c] + rh[c]);
        sh[c] = 0.5 * ((K[3][c] - K[0][c]) + (K[4][c] - K[0][c]));
        ex[c] = rh[c] - lh[c];
        ey[c] = sh[c] - hips[c];
    }
    const double s = torso ? norm3(ey[0], ey[1], ey[2]) : norm3(ex[0], ex[1], ex[2]);
    unit3(ex, 1e-9);
    unit3(ey, 1e-9);
    ez[0] = ex[1] * ey[2] - ex[2] * ey[1], ez[1] = ex[2] * ey[0] - ex[0] * ey[2], ez[2] = ex[0] * ey[1] - ex[1] * ey[0];
    unit3(ez, 1e-9);
    ey[0] = ez[1] * ex[2] - ez[2] * ex[1], ey[1] = ez[2] * ex[0] - ez[0] * ex[2], ey[2] = ez[0] * ex[1] - ez[1] * ex[0];
    unit3(ey, 1e-9);
    ok = ok && is_fin(s) && !(s < 1e-9);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const double x0 = X[k][0] - K[0][0], x1 = X[k][1] - K[0][1], x2 = X[k][2] - K[0][2];
        C[k][0] = ok ? (ex[0] * x0 + ex[1] * x1 + ex[2] * x2) / s : nan;
        C[k][1] = ok ? (ey[0] * x0 + ey[1] * x1 + ey[2] * x2) / s : nan;
        C[k][2] = ok ? (ez[0] * x0 + ez[1] * x1 + ez[2] * x2) / s : nan;
    }
}

// the lane's rows (joints lane and lane + 64) of frame `row0 / J` of one view: NaN beyond J; U may be NULL (then not read)
__device__ inline void load_rows(const double* X, const double* U, long row0, int J, int lane, bool* act, double (*Xo)[3],
                                 double (*Uo)[2]) {
    const double nan = qnan();
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int j = lane + 64 * k;
        act[k] = j < J;
        const long row = row0 + (act[k] ? j : 0);
#pragma unroll
        for (int c = 0; c < 3; ++c) Xo[k][c] = act[k] ? X[row * 3 + c] : nan;
        if (U) {
#pragma unroll
            for (int c = 0; c < 2; ++c) Uo[k][c] = act[k] ? U[row * 2 + c] : nan;
        }
    }
}

// align_right_to_left: Kabsch right -> left on the joints finite in both; fewer than 3: the right view unchanged
__device__ inline void kabsch_align(const double (*Xl)[3], const double (*Xr)[3], const bool* act, double (*Al)[3]) {
    bool both[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) both[k] = act[k] && fin3(Xl[k]) && fin3(Xr[k]);
    const double nb = wave_sum((both[0] ? 1.0 : 0.0) + (both[1] ? 1.0 : 0.0));
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
        for (int c = 0; c < 3; ++c) Al[k][c] = Xr[k][c];
    if (nb >= 3.0) {
        double cs[3], cd[3], H[9], P[9], ssum, tv[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            cs[c] = wave_sum((both[0] ? Xr[0][c] : 0.0) + (both[1] ? Xr[1][c] : 0.0)) / nb;
            cd[c] = wave_sum((both[0] ? Xl[0][c] : 0.0) + (both[1] ? Xl[1][c] : 0.0)) / nb;
        }
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c)
                H[3 * r + c] = wave_sum((both[0] ? (Xr[0][r] - cs[r]) * (Xl[0][c] - cd[c]) : 0.0) +
                                    (both[1] ? (Xr[1][r] - cs[r]) * (Xl[1][c] - cd[c]) : 0.0));
        polar3(H, P, ssum);                    // R = V U^T = P^T
#pragma unroll
        for (int r = 0; r < 3; ++r) tv[r] = cd[r] - (P[r] * cs[0] + P[3 + r] * cs[1] + P[6 + r] * cs[2]);
#pragma unroll
        for (int k = 0; k < 2; ++k)
#pragma unroll
            for (int r = 0; r < 3; ++r)
                if (both[k]) Al[k][r] = (Xr[k][0] * P[r] + Xr[k][1] * P[3 + r] + Xr[k][2] * P[6 + r]) + tv[r];
    }
}

// crossview_consistency_confidence of one joint from its two canonical rows -> dist (NaN where either is), conf_x
__device__ inline void cross_conf(const double* Ca, const double* Cb, double var3, double& d, double& cx) {
    const bool ok = fin3(Ca) && fin3(Cb);
    const double d0 = Ca[0] - Cb[0], d1 = Ca[1] - Cb[1], d2 = Ca[2] - Cb[2];
    d = ok ? sqrt(d0 * d0 + d1 * d1 + d2 * d2) : qnan();
    cx = is_fin(d) ? exp(-(d * d) / (2.0 * var3)) : 0.0;
}

// fuse_frame_3d of one joint: softmax2 of the qualities, then (left present) + 2 (right present)
__device__ inline void fuse_row(double ql, double qr, const double* Xl, const double* Al, double* F) {
    const double nan = qnan();
    const double m = (ql != ql || qr != qr) ? nan : fmax(ql, qr);
    const double ea = exp(ql - m), eb = exp(qr - m), se = ea + eb + 1e-8;
    const double wl = ea / se, wr = eb / se;
    const bool lok = fin3(Xl), rok = fin3(Al);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double blend = (wl * Xl[c] + wr * Al[c]) / (wl + wr + 1e-8);
        F[c] = lok ? (rok ? blend : Xl[c]) : (rok ? Al[c] : nan);
    }
}

__global__ __launch_bounds__(256) void fuse_views_kernel(ViewsArgs a) {
    const int lane = threadIdx.x & 63;
    const long t = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= a.T) return;                      // the whole wave leaves: no barrier in this kernel
    const int J = a.J;
    bool act[2];
    double Xl[2][3], Xr[2][3], Ul[2][2], Ur[2][2], Al[2][3];
    load_rows(a.Xl, a.Ul, t * J, J, lane, act, Xl, Ul);
    load_rows(a.Xr, a.Ur, t * J, J, lane, act, Xr, Ur);
    kabsch_align(Xl, Xr, act, Al);
    // the confidences, each view on its raw 3D
    double cl[2], cr[2], el[2], er[2], Ca[2][3], Cb[2][3];
    const bool okl = weakpersp(Xl, Ul, act, a.min_points, a.sigma_px, cl, el);
    const bool okr = weakpersp(Xr, Ur, act, a.min_points, a.sigma_px, cr, er);
    canonicalize(a.Xl + t * J * 3, a.key, a.torso, Xl, Ca);
    canonicalize(a.Xr + t * J * 3, a.key, a.torso, Xr, Cb);
    const double s3 = fmax(a.sigma_3d, 1e-12), var3 = s3 * s3;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        if (!act[k]) continue;
        double d, cx, F[3];
        cross_conf(Ca[k], Cb[k], var3, d, cx);
        const double ql = sqrt(cl[k] * cx), qr = sqrt(cr[k] * cx);
        fuse_row(ql, qr, Xl[k], Al[k], F);
        const long row = t * J + lane + 64 * k;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            a.fused[row * 3 + c] = F[c];
            a.aligned[row * 3 + c] = Al[k][c];
        }
        a.q_l[row] = ql, a.q_r[row] = qr;
        a.conf_l[row] = cl[k], a.conf_r[row] = cr[k], a.conf_x[row] = cx;
        a.err_l[row] = el[k], a.err_r[row] = er[k], a.dist[row] = d;
    }
    if (lane == 0) {
        a.fit_ok[2 * t] = okl ? 1 : 0;
        a.fit_ok[2 * t + 1] = okr ? 1 : 0;
    }
}

// ---- fusion of a camera group (fuse/main_unity.py:98-132, fuse/main_raw.py:194-240): every pair of V views ------------
// Two kernels.  group_views_kernel, one wave per (view, frame): the view's weak-perspective confidence and its canonical
// pose (workspace), once each.  group_pairs_kernel, one wave per (pair, frame), pairs in itertools.combinations order: the
// Kabsch alignment (align), the cross-view confidence from the two canonical poses, fuse_frame_3d.  The arithmetic is
// fuse_views_kernel's, through the same device functions, so a pair's results are that kernel's bit for bit.
struct GroupArgs {
    const double *X, *U, *Q;                   // [V, T, J, 3], [V, T, J, 2], given qualities [V, T, J] or NULL
    double *canon, *conf, *err;                // workspace [V, T, J, 3]; [V, T, J]
    int32_t* fit_ok;                           // [V, T]
    double *fused, *aligned, *q_a, *q_b, *conf_x, *dist;
    long V, T, P;
    int J, key[5], torso, min_points, align;
    double sigma_px, sigma_3d;
};

__global__ __launch_bounds__(256) void group_views_kernel(GroupArgs a) {
    const int lane = threadIdx.x & 63;
    const long w = (long)blockIdx.x * 4 + (threadIdx.x >> 6);        // = view * T + frame
    if (w >= a.V * a.T) return;
    const int J = a.J;
    bool act[2];
    double X[2][3], U[2][2], cf[2], er[2], Cn[2][3];
    load_rows(a.X, a.U, w * J, J, lane, act, X, U);
    const bool ok = weakpersp(X, U, act, a.min_points, a.sigma_px, cf, er);
    canonicalize(a.X + w * J * 3, a.key, a.torso, X, Cn);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        if (!act[k]) continue;
        const long row = w * J + lane + 64 * k;
        a.conf[row] = cf[k], a.err[row] = er[k];
#pragma unroll
        for (int c = 0; c < 3; ++c) a.canon[row * 3 + c] = Cn[k][c];
    }
    if (lane == 0) a.fit_ok[w] = ok ? 1 : 0;
}

__global__ __launch_bounds__(256) void group_pairs_kernel(GroupArgs a) {
    const int lane = threadIdx.x & 63;
    const long w = (long)blockIdx.x * 4 + (threadIdx.x >> 6);        // = pair * T + frame
    if (w >= a.P * a.T) return;
    const long p = w / a.T, t = w - p * a.T;
    long va = 0, rem = p;                      // pair p of combinations(range(V), 2)
    while (rem >= a.V - 1 - va) rem -= a.V - 1 - va, ++va;
    const long vb = va + 1 + rem;
    const int J = a.J;
    const long ra = (va * a.T + t) * J, rb = (vb * a.T + t) * J;
    bool act[2];
    double Xa[2][3], Xb[2][3], Al[2][3];
    load_rows(a.X, nullptr, ra, J, lane, act, Xa, nullptr);
    load_rows(a.X, nullptr, rb, J, lane, act, Xb, nullptr);
    if (a.align) {
        kabsch_align(Xa, Xb, act, Al);
    } else {
#pragma unroll
        for (int k = 0; k < 2; ++k)
#pragma unroll
            for (int c = 0; c < 3; ++c) Al[k][c] = Xb[k][c];
    }
    const double s3 = fmax(a.sigma_3d, 1e-12), var3 = s3 * s3;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        if (!act[k]) continue;
        const int j = lane + 64 * k;
        const long row = w * J + j;
        double qa, qb, F[3];
        if (a.Q) {
            qa = a.Q[ra + j], qb = a.Q[rb + j];
        } else {
            double d, cx;
            cross_conf(a.canon + (ra + j) * 3, a.canon + (rb + j) * 3, var3, d, cx);
            qa = sqrt(a.conf[ra + j] * cx), qb = sqrt(a.conf[rb + j] * cx);
            a.conf_x[row] = cx, a.dist[row] = d;
        }
        fuse_row(qa, qb, Xa[k], Al[k], F);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            a.fused[row * 3 + c] = F[c];
            a.aligned[row * 3 + c] = Al[k][c];
        }
        a.q_a[row] = qa, a.q_b[row] = qb;
    }
}

// ---- ground-truth-free joint quality (fuse/fuse.py:124-285) -----------------------------------------------------------
struct QualityArgs {
    const double *X, *U, *size, *bias;         // [V, T, J, 3]; [V, T, J, 2] or NULL; [V, 2] (width, height); [J] / [V, J] or NULL
    const int32_t* edges;                      // [E, 2]
    double *med, *q, *q_bone, *q_temp, *q_san; // [V, E]; [V, T, J] each
    long V, T, bias_stride;
    int J, E;
    double beta, w_bone, w_temp, w_san;
};

// the order-preserving key of edge (ia, ib)'s length in the frame whose first row is row0; 0 where a row is not finite
// (a length is >= +0, so every real key has its top bit set)
__device__ inline unsigned long long edge_key(const double* X, long row0, int ia, int ib) {
    const double *pa = X + (row0 + ia) * 3, *pb = X + (row0 + ib) * 3;
    if (!(fin3(pa) && fin3(pb))) return 0ULL;
    return key64(norm3(pa[0] - pb[0], pa[1] - pb[1], pa[2] - pb[2]));
}

// NaN-ignoring median of an edge's lengths over the clip: one wave per (view, edge), lanes over frames, the exact selection
// of the two middle ranks over the keys (reduce.h: wave_select2, shared with evaluate.hip's per-joint medians).  The first
// kKeyCache keys of a lane stay in registers; longer clips recompute the rest in every pass.
constexpr int kKeyCache = 4;
__global__ __launch_bounds__(256) void bone_median_kernel(QualityArgs a) {
    const int lane = threadIdx.x & 63;
    const long w = (long)blockIdx.x * 4 + (threadIdx.x >> 6);        // = view * E + edge
    if (w >= a.V * a.E) return;
    const long v = w / a.E;
    const int e = (int)(w - v * a.E), J = a.J;
    const int ia = a.edges[2 * e], ib = a.edges[2 * e + 1];
    if (ia < 0 || ia >= J || ib < 0 || ib >= J) {                    // the reference's `a not in idx`: no sample at all
        if (lane == 0) a.med[w] = qnan();
        return;
    }
    const long T = a.T, f0 = v * T;
    unsigned long long kc[kKeyCache];
    unsigned cnt = 0;
#pragma unroll
    for (int k = 0; k < kKeyCache; ++k) {
        const long t = lane + 64 * k;
        kc[k] = t < T ? edge_key(a.X, (f0 + t) * J, ia, ib) : 0ULL;
        cnt += (unsigned)(kc[k] >> 63);
    }
    for (long t = lane + 64 * kKeyCache; t < T; t += 64) cnt += (unsigned)(edge_key(a.X, (f0 + t) * J, ia, ib) >> 63);
    const unsigned n = wave_sum(cnt);
    if (n == 0) {
        if (lane == 0) a.med[w] = qnan();
        return;
    }
    unsigned long long p0, p1;               // a missing sample's key is 0 and takes no part
    wave_select2((n - 1) / 2, n / 2, [&](auto&& f) {
#pragma unroll
        for (int k = 0; k < kKeyCache; ++k)
            if (kc[k] >> 63) f(kc[k]);
        for (long t = lane + 64 * kKeyCache; t < T; t += 64) {
            const unsigned long long key = edge_key(a.X, (f0 + t) * J, ia, ib);
            if (key >> 63) f(key);
        }
    }, p0, p1);
    const double lo = unkey64(p0), hi = unkey64(p1);
    if (lane == 0) a.med[w] = (n & 1u) ? lo : (lo + hi) / 2.0;
}

// one wave per (view, frame), lanes over joints: a lane walks the edge list in its order for each of its joints
__global__ __launch_bounds__(256) void joint_quality_kernel(QualityArgs a) {
    const int lane = threadIdx.x & 63;
    const long w = (long)blockIdx.x * 4 + (threadIdx.x >> 6);        // = view * T + frame
    if (w >= a.V * a.T) return;
    const long v = w / a.T, t = w - v * a.T;
    const int J = a.J;
    const double* F = a.X + w * J * 3;
    const double* med = a.med + v * a.E;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int j = lane + 64 * k;
        if (j >= J) continue;
        const double* x = F + 3 * j;
        const bool ok = fin3(x);
        double qb = -1e9, qt = -1e9, qs = -50.0;
        if (ok) {
            double dev = 0.0;
            int cnt = 0;
            for (int e = 0; e < a.E; ++e) {
                const int ia = a.edges[2 * e], ib = a.edges[2 * e + 1];
                if (ia < 0 || ia >= J || ib < 0 || ib >= J || !is_fin(med[e])) continue;
                if (ia == j) {
                    const double* o = F + 3 * ib;
                    if (fin3(o)) dev += fabs(norm3(x[0] - o[0], x[1] - o[1], x[2] - o[2]) - med[e]), ++cnt;
                }
                if (ib == j) {                                       // a self-edge counts twice, as in the reference
                    const double* o = F + 3 * ia;
                    if (fin3(o)) dev += fabs(norm3(x[0] - o[0], x[1] - o[1], x[2] - o[2]) - med[e]), ++cnt;
                }
            }
            qb = cnt == 0 ? -100.0 : -(dev / ((double)cnt + 1e-8));
            qt = 0.0;
            if (t > 0) {
                const double* p = x - (long)J * 3;
                if (fin3(p)) qt = -a.beta * norm3(x[0] - p[0], x[1] - p[1], x[2] - p[2]);
            }
        }
        if (a.U) {
            const double u0 = a.U[(w * J + j) * 2], u1 = a.U[(w * J + j) * 2 + 1];
            const double W = a.size[2 * v], H = a.size[2 * v + 1];
            if (is_fin(u0) && is_fin(u1) && 0.0 <= u0 && u0 < W && 0.0 <= u1 && u1 < H) qs = 0.0;
        }
        double q = (a.w_bone * qb + a.w_temp * qt) + a.w_san * qs;
        if (a.bias) q = q + a.bias[v * a.bias_stride + j];
        const long row = w * J + j;
        a.q[row] = q, a.q_bone[row] = qb, a.q_temp[row] = qt, a.q_san[row] = qs;
    }
}

// ---- temporal_smooth_ema: one thread per joint ----------------------------------------------------------------------
// the walk of joint j over the clip X [T, J, 3] -> Y
__device__ inline void ema_walk(const double* __restrict__ X, long T, long J, long j, const double* __restrict__ base, int adaptive,
                                double amin, double amax, double gain, double* __restrict__ Y) {
    const double nan = qnan();
    const double b = base[j];
    double st[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) Y[j * 3 + c] = st[c] = X[j * 3 + c];
    bool has = fin3(st);
    for (long t0 = 1; t0 < T; t0 += kBatch) {
        double xb[kBatch][3];
#pragma unroll
        for (int i = 0; i < kBatch; ++i)
#pragma unroll
            for (int c = 0; c < 3; ++c) xb[i][c] = t0 + i < T ? X[((t0 + i) * J + j) * 3 + c] : nan;
#pragma unroll
        for (int i = 0; i < kBatch; ++i) {
            if (t0 + i >= T) break;
            const double* x = xb[i];
            const bool obs = fin3(x);
            double y[3];
            if (obs && has) {
                const double d0 = x[0] - st[0], d1 = x[1] - st[1], d2 = x[2] - st[2];
                const double al = adaptive ? fmin(fmax(b + gain * sqrt(d0 * d0 + d1 * d1 + d2 * d2), amin), amax) : b;
#pragma unroll
                for (int c = 0; c < 3; ++c) y[c] = al * x[c] + (1.0 - al) * st[c];
            } else {
#pragma unroll
                for (int c = 0; c < 3; ++c) y[c] = obs ? x[c] : (has ? st[c] : nan);
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) Y[((t0 + i) * J + j) * 3 + c] = st[c] = y[c];
            has = fin3(st);
        }
    }
}

__global__ __launch_bounds__(64) void smooth_ema_kernel(const double* __restrict__ X, long T, long J, const double* __restrict__ base,
                                                        int adaptive, double amin, double amax, double gain, double* __restrict__ Y) {
    const long j = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= J) return;
    ema_walk(X, T, J, j, base, adaptive, amin, amax, gain, Y);
}

// B clips [B, T, J, 3] with one base [J]: one thread per (clip, joint), the same walk
__global__ __launch_bounds__(64) void smooth_ema_batch_kernel(const double* __restrict__ X, long B, long T, long J,
                                                              const double* __restrict__ base, int adaptive, double amin, double amax,
                                                              double gain, double* __restrict__ Y) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * J) return;
    const long b = i / J;
    ema_walk(X + b * T * J * 3, T, J, i - b * J, base, adaptive, amin, amax, gain, Y + b * T * J * 3);
}

// ---- smooth_skeleton: one thread per (joint, coordinate) series -----------------------------------------------------
// The finite samples of a series form one contiguous sequence x_0 .. x_{n-1}.  Sample k goes to slot k % win of the
// thread's ring (values and time indices, LDS, [slot][thread]); once `win` samples are in, every new sample completes the
// window of the sample win / 2 behind it.  The first and the last window also give the win / 2 edge samples.
// WIN: the window as a compile-time constant (the loops over it unroll and the FIR row stays in registers), or 0 for any
// window up to kMaxWin; the arithmetic and its order are the same.
template <int WIN>
__global__ __launch_bounds__(64) void smooth_savgol_kernel(const double* __restrict__ X, long T, long S, int win_arg, const double* __restrict__ fir,
                                                           const double* __restrict__ first, const double* __restrict__ last,
                                                           double* __restrict__ Y) {
    const int win = WIN ? WIN : win_arg;
    __shared__ double ring[WIN ? WIN : kMaxWin][64];
    __shared__ int ring_t[WIN ? WIN : kMaxWin][64];
    const int tid = threadIdx.x;
    const long s = (long)blockIdx.x * 64 + tid;
    if (s >= S) return;                        // no barrier in this kernel: a thread owns its ring columns
    const int half = win / 2;
    long n = 0;
    for (long t0 = 0; t0 < T; t0 += kBatch) {
        double xb[kBatch];
#pragma unroll
        for (int i = 0; i < kBatch; ++i) xb[i] = t0 + i < T ? X[(t0 + i) * S + s] : qnan();
#pragma unroll
        for (int i = 0; i < kBatch; ++i) n += is_fin(xb[i]) ? 1 : 0;
    }
    const bool filter = n >= win;
    long k = 0;
    int head = 0;                              // k % win: the slot of the next sample = of the window's oldest
    for (long t0 = 0; t0 < T; t0 += kBatch) {
        double xb[kBatch];
#pragma unroll
        for (int i = 0; i < kBatch; ++i) xb[i] = t0 + i < T ? X[(t0 + i) * S + s] : 0.0;
#pragma unroll
        for (int i = 0; i < kBatch; ++i) {
            const long t = t0 + i;
            if (t >= T) break;
            const double x = xb[i];
            if (!filter || !is_fin(x)) {
                Y[t * S + s] = x;
                continue;
            }
            ring[head][tid] = x;
            ring_t[head][tid] = (int)t;
            head = head + 1 == win ? 0 : head + 1;
            ++k;
            if (k < win) continue;
            // the window: element m at slot (head + m) % win
            if (k == win)
                for (int e = 0; e < half; ++e) {
                    double acc = 0.0;
                    int p = head;
                    for (int m = 0; m < win; ++m) {
                        acc += first[e * win + m] * ring[p][tid];
                        p = p + 1 == win ? 0 : p + 1;
                    }
                    const int pe = head + e >= win ? head + e - win : head + e;
                    Y[(long)ring_t[pe][tid] * S + s] = acc;
                }
            {
                double acc = 0.0;
                int p = head;
                for (int m = 0; m < win; ++m) {
                    acc += fir[m] * ring[p][tid];
                    p = p + 1 == win ? 0 : p + 1;
                }
                const int pc = head + half >= win ? head + half - win : head + half;
                Y[(long)ring_t[pc][tid] * S + s] = acc;
            }
            if (k == n)
                for (int e = 0; e < half; ++e) {
                    double acc = 0.0;
                    int p = head;
                    for (int m = 0; m < win; ++m) {
                        acc += last[e * win + m] * ring[p][tid];
                        p = p + 1 == win ? 0 : p + 1;
                    }
                    const int o = head + half + 1 + e;
                    const int pe = o >= win ? o - win : o;
                    Y[(long)ring_t[pe][tid] * S + s] = acc;
                }
        }
    }
}

constexpr long kMaxElems = 1L << 40;          // T * J: every offset 3 (T J) + 2 stays far inside 63 bits

}  // namespace
}  // namespace skimi

using namespace skimi;

extern "C" {

int skimi_fuse_h36m(const double* left, const double* right, int64_t frames, double tau, const double* tau_j, const double* wL,
                    int64_t wL_stride, const double* wR, int64_t wR_stride, int32_t allow_scale, int32_t mirror_right_x,
                    double* fused, double* R, double* t, double* s, double* diag, int32_t* status, void* stream) {
    SKIMI_CHECK_ARG(frames >= 0 && frames <= kMaxElems / kH36mJoints, "skimi_fuse_h36m: frames = %lld outside 0..2^40 / 17", (long long)frames);
    SKIMI_CHECK_ARG((wL_stride == 0 || wL_stride == kH36mJoints) && (wR_stride == 0 || wR_stride == kH36mJoints),
                    "skimi_fuse_h36m: weight strides %lld, %lld are neither 0 ([17]) nor 17 ([frames, 17])", (long long)wL_stride,
                    (long long)wR_stride);
    if (frames == 0) return SKIMI_OK;
    SKIMI_CHECK_ARG(left && right, "skimi_fuse_h36m: NULL input");
    SKIMI_CHECK_ARG(fused && R && t && s && diag && status, "skimi_fuse_h36m: NULL output");
    H36mArgs a{};
    a.left = left, a.right = right, a.tau_j = tau_j, a.wL = wL, a.wR = wR;
    a.fused = fused, a.R = R, a.t = t, a.s = s, a.diag = diag, a.status = status;
    a.T = frames, a.wL_stride = wL_stride, a.wR_stride = wR_stride, a.tau = tau;
    a.allow_scale = allow_scale != 0, a.mirror = mirror_right_x != 0;
    hipLaunchKernelGGL(fuse_h36m_kernel, dim3((unsigned)cdiv(frames, 4)), dim3(256), 0, (hipStream_t)stream, a);
    SKIMI_LAUNCH_CHECK();
    return SKIMI_OK;
}

int skimi_fuse_views(const double* X_l, const double* X_r, const double* U_l, const double* U_r, int64_t frames, int32_t joints,
                     int32_t root_idx, int32_t left_hip_idx, int32_t right_hip_idx, int32_t left_shoulder_idx,
                     int32_t right_shoulder_idx, double sigma_px, double sigma_3d, int32_t scale_mode, int32_t min_points,
                     double* fused, double* aligned, double* q_l, double* q_r, double* conf_l, double* conf_r, double* conf_x,
                     double* err_l, double* err_r, double* dist, int32_t* fit_ok, void* stream) {
    SKIMI_CHECK_ARG(joints >= 1 && joints <= kMaxJoints, "skimi_fuse_views: joints = %d outside 1..%d", joints, kMaxJoints);
    SKIMI_CHECK_ARG(frames >= 0 && frames <= kMaxElems / kMaxJoints, "skimi_fuse_views: frames = %lld outside 0..2^33", (long long)frames);
    const int32_t key[5] = {root_idx, left_hip_idx, right_hip_idx, left_shoulder_idx, right_shoulder_idx};
    for (int i = 0; i < 5; ++i)
        SKIMI_CHECK_ARG(key[i] >= 0 && key[i] < joints, "skimi_fuse_views: key joint %d = %d outside 0..%d", i, key[i], joints - 1);
    SKIMI_CHECK_ARG(fabs(sigma_px) <= 1.79769313486231570815e308 && fabs(sigma_3d) <= 1.79769313486231570815e308,
                    "skimi_fuse_views: sigma_px = %g, sigma_3d = %g must be finite", sigma_px, sigma_3d);
    SKIMI_CHECK_ARG(scale_mode == SKIMI_FUSE_SCALE_HIP || scale_mode == SKIMI_FUSE_SCALE_TORSO, "skimi_fuse_views: unknown scale_mode %d",
                    scale_mode);
    SKIMI_CHECK_ARG(min_points >= 1, "skimi_fuse_views: min_points = %d < 1", min_points);
    if (frames == 0) return SKIMI_OK;
    SKIMI_CHECK_ARG(X_l && X_r && U_l && U_r, "skimi_fuse_views: NULL input");
    SKIMI_CHECK_ARG(fused && aligned && q_l && q_r && conf_l && conf_r && conf_x && err_l && err_r && dist && fit_ok,
                    "skimi_fuse_views: NULL output");
    ViewsArgs a{};
    a.Xl = X_l, a.Xr = X_r, a.Ul = U_l, a.Ur = U_r;
    a.fused = fused, a.aligned = aligned, a.q_l = q_l, a.q_r = q_r, a.conf_l = conf_l, a.conf_r = conf_r, a.conf_x = conf_x;
    a.err_l = err_l, a.err_r = err_r, a.dist = dist, a.fit_ok = fit_ok;
    a.T = frames, a.J = joints, a.torso = scale_mode == SKIMI_FUSE_SCALE_TORSO, a.min_points = min_points;
    for (int i = 0; i < 5; ++i) a.key[i] = key[i];
    a.sigma_px = sigma_px, a.sigma_3d = sigma_3d;
    hipLaunchKernelGGL(fuse_views_kernel, dim3((unsigned)cdiv(frames, 4)), dim3(256), 0, (hipStream_t)stream, a);
    SKIMI_LAUNCH_CHECK();
    return SKIMI_OK;
}

int skimi_smooth_ema(const double* X, int64_t frames, int64_t joints, const double* base, int32_t adaptive, double alpha_min,
                     double alpha_max, double speed_gain, double* Y, void* stream) {
    SKIMI_CHECK_ARG(frames >= 0 && joints >= 0 && joints <= 0x7fffffffLL && (joints == 0 || frames <= kMaxElems / joints),
                    "skimi_smooth_ema: frames = %lld, joints = %lld outside frames, joints >= 0, frames * joints <= 2^40",
                    (long long)frames, (long long)joints);
    if (frames == 0 || joints == 0) return SKIMI_OK;
    SKIMI_CHECK_ARG(X && base && Y && X != Y, "skimi_smooth_ema: NULL input or output, or Y is X");
    hipLaunchKernelGGL(smooth_ema_kernel, dim3((unsigned)cdiv(joints, 64)), dim3(64), 0, (hipStream_t)stream, X, (long)frames,
                       (long)joints, base, adaptive != 0, alpha_min, alpha_max, speed_gain, Y);
    SKIMI_LAUNCH_CHECK();
    return SKIMI_OK;
}

int skimi_smooth_ema_batch(const double* X, int64_t clips, int64_t frames, int64_t joints, const double* base, int32_t adaptive,
                           double alpha_min, double alpha_max, double speed_gain, double* Y, void* stream) {
    SKIMI_CHECK_ARG(clips >= 0 && frames >= 0 && joints >= 0 && joints <= 0x7fffffffLL && clips <= 0x7fffffffLL &&
                        (joints == 0 || clips == 0 || frames <= kMaxElems / joints / clips),
                    "skimi_smooth_ema_batch: clips = %lld, frames = %lld, joints = %lld outside clips, frames, joints >= 0, clips * "
                    "frames * joints <= 2^40", (long long)clips, (long long)frames, (long long)joints);
    if (clips == 0 || frames == 0 || joints == 0) return SKIMI_OK;
    SKIMI_CHECK_ARG(X && base && Y && X != Y, "skimi_smooth_ema_batch: NULL input or output, or Y is X");
    hipLaunchKernelGGL(smooth_ema_batch_kernel, dim3((unsigned)cdiv(clips * joints, 64)), dim3(64), 0, (hipStream_t)stream, X,
                       (long)clips, (long)frames, (long)joints, base, adaptive != 0, alpha_min, alpha_max, speed_gain, Y);
    SKIMI_LAUNCH_CHECK();
    return SKIMI_OK;
}

size_t skimi_fuse_group_workspace_bytes(int64_t views, int64_t frames, int32_t joints) {
    if (views < 0 || frames < 0 || joints < 1 || joints > kMaxJoints) return 0;
    if (views > 0 && frames > 0x7fffffffLL / views) return 0;
    return (size_t)views * (size_t)frames * (size_t)joints * 3 * sizeof(double);
}

int skimi_fuse_group(const double* X, const double* U, const double* quality, int64_t views, int64_t frames, int32_t joints,
                     int32_t root_idx, int32_t left_hip_idx, int32_t right_hip_idx, int32_t left_shoulder_idx,
                     int32_t right_shoulder_idx, double sigma_px, double sigma_3d, int32_t scale_mode, int32_t min_points,
                     int32_t align, void* workspace, size_t workspace_bytes, double* fused, double* aligned, double* q_a, double* q_b,
                     double* conf_x, double* dist, double* conf, double* err, int32_t* fit_ok, void* stream) {
    SKIMI_CHECK_ARG(joints >= 1 && joints <= kMaxJoints, "skimi_fuse_group: joints = %d outside 1..%d", joints, kMaxJoints);
    SKIMI_CHECK_ARG(views >= 0 && views <= 4096, "skimi_fuse_group: views = %lld outside 0..4096", (long long)views);
    const int64_t pairs = views * (views - 1) / 2;
    SKIMI_CHECK_ARG(frames >= 0 && (pairs == 0 || frames <= 0x7fffffffLL / pairs) && (views == 0 || frames <= 0x7fffffffLL / views),
                    "skimi_fuse_group: frames = %lld: frames * views and frames * pairs must stay below 2^31", (long long)frames);
    const int32_t key[5] = {root_idx, left_hip_idx, right_hip_idx, left_shoulder_idx, right_shoulder_idx};
    for (int i = 0; i < 5; ++i)
        SKIMI_CHECK_ARG(key[i] >= 0 && key[i] < joints, "skimi_fuse_group: key joint %d = %d outside 0..%d", i, key[i], joints - 1);
    SKIMI_CHECK_ARG(fabs(sigma_px) <= 1.79769313486231570815e308 && fabs(sigma_3d) <= 1.79769313486231570815e308,
                    "skimi_fuse_group: sigma_px = %g, sigma_3d = %g must be finite", sigma_px, sigma_3d);
    SKIMI_CHECK_ARG(scale_mode == SKIMI_FUSE_SCALE_HIP || scale_mode == SKIMI_FUSE_SCALE_TORSO, "skimi_fuse_group: unknown scale_mode %d",
                    scale_mode);
    SKIMI_CHECK_ARG(min_points >= 1, "skimi_fuse_group: min_points = %d < 1", min_points);
    if (frames == 0 || views == 0) return SKIMI_OK;
    SKIMI_CHECK_ARG(X, "skimi_fuse_group: NULL input");
    GroupArgs a{};
    a.X = X, a.U = U, a.Q = quality;
    a.canon = (double*)workspace, a.conf = conf, a.err = err, a.fit_ok = fit_ok;
    a.fused = fused, a.aligned = aligned, a.q_a = q_a, a.q_b = q_b, a.conf_x = conf_x, a.dist = dist;
    a.V = views, a.T = frames, a.P = pairs, a.J = joints;
    a.torso = scale_mode == SKIMI_FUSE_SCALE_TORSO, a.min_points = min_points, a.align = align != 0;
    for (int i = 0; i < 5; ++i) a.key[i] = key[i];
    a.sigma_px = sigma_px, a.sigma_3d = sigma_3d;
    if (!quality) {
        SKIMI_CHECK_ARG(U && conf && err && fit_ok, "skimi_fuse_group: without given qualities U, conf, err and fit_ok are needed");
        SKIMI_CHECK_ARG(pairs == 0 || (conf_x && dist), "skimi_fuse_group: NULL conf_x or dist");
        SKIMI_CHECK_ARG(workspace && workspace_bytes >= skimi_fuse_group_workspace_bytes(views, frames, joints),
                        "skimi_fuse_group: the workspace is NULL or smaller than skimi_fuse_group_workspace_bytes");
        hipLaunchKernelGGL(group_views_kernel, dim3((unsigned)cdiv(views * frames, 4)), dim3(256), 0, (hipStream_t)stream, a);
        SKIMI_LAUNCH_CHECK();
    }
    if (pairs == 0) return SKIMI_OK;
    SKIMI_CHECK_ARG(fused && aligned && q_a && q_b, "skimi_fuse_group: NULL pair output");
    hipLaunchKernelGGL(group_pairs_kernel, dim3((unsigned)cdiv(pairs * frames, 4)), dim3(256), 0, (hipStream_t)stream, a);
    SKIMI_LAUNCH_CHECK();
    return SKIMI_OK;
}

int skimi_joint_quality(const double* X, const double* U, int64_t views, int64_t frames, int32_t joints, const int32_t* edges,
                        int32_t n_edges, const double* size, double beta_temp, double w_bone, double w_temp, double w_san,
                        int32_t med_given, const double* bias, int64_t bias_stride, double* med_lens, double* q, double* q_bone,
                        double* q_temp, double* q_san, void* stream) {
    SKIMI_CHECK_ARG(joints >= 1 && joints <= kMaxJoints, "skimi_joint_quality: joints = %d outside 1..%d", joints, kMaxJoints);
    SKIMI_CHECK_ARG(views >= 0 && views <= 4096 && n_edges >= 0 && n_edges <= 65536,
                    "skimi_joint_quality: views = %lld, n_edges = %d outside 0..4096, 0..65536", (long long)views, n_edges);
    SKIMI_CHECK_ARG(frames >= 0 && (views == 0 || frames <= 0x7fffffffLL / views),
                    "skimi_joint_quality: frames = %lld: views * frames must stay below 2^31", (long long)frames);
    SKIMI_CHECK_ARG(bias_stride == 0 || bias_stride == joints, "skimi_joint_quality: bias_stride = %lld is neither 0 ([joints]) nor joints "
                    "([views, joints])", (long long)bias_stride);
    if (views == 0) return SKIMI_OK;
    SKIMI_CHECK_ARG(n_edges == 0 || (edges && med_lens), "skimi_joint_quality: NULL edges or med_lens");
    QualityArgs a{};
    a.X = X, a.U = U, a.size = size, a.bias = bias, a.edges = edges;
    a.med = med_lens, a.q = q, a.q_bone = q_bone, a.q_temp = q_temp, a.q_san = q_san;
    a.V = views, a.T = frames, a.bias_stride = bias_stride, a.J = joints, a.E = n_edges;
    a.beta = beta_temp, a.w_bone = w_bone, a.w_temp = w_temp, a.w_san = w_san;
    SKIMI_CHECK_ARG(frames == 0 || (X && q && q_bone && q_temp && q_san && (!U || size)),
                    "skimi_joint_quality: NULL input or output, or U without size");
    if (n_edges > 0 && !med_given) {           // frames == 0: every median is NaN, written by the same kernel
        hipLaunchKernelGGL(bone_median_kernel, dim3((unsigned)cdiv(views * n_edges, 4)), dim3(256), 0, (hipStream_t)stream, a);
        SKIMI_LAUNCH_CHECK();
    }
    if (frames == 0) return SKIMI_OK;
    hipLaunchKernelGGL(joint_quality_kernel, dim3((unsigned)cdiv(views * frames, 4)), dim3(256), 0, (hipStream_t)stream, a);
    SKIMI_LAUNCH_CHECK();
    return SKIMI_OK;
}

int skimi_smooth_savgol(const double* X, int64_t frames, int64_t joints, int32_t win, int32_t poly, const double* fir,
                        const double* first, const double* last, double* Y, void* stream) {
    SKIMI_CHECK_ARG(frames >= 0 && frames <= 0x7fffffffLL && joints >= 0 && joints <= 0x7fffffffLL / 3 &&
                        (joints == 0 || frames <= kMaxElems / joints),
                    "skimi_smooth_savgol: frames = %lld, joints = %lld outside 0 <= frames < 2^31, joints >= 0, frames * joints <= 2^40",
                    (long long)frames, (long long)joints);
    SKIMI_CHECK_ARG(win >= 1 && win <= kMaxWin && win % 2 == 1, "skimi_smooth_savgol: win = %d is not an odd number in 1..%d", win, kMaxWin);
    SKIMI_CHECK_ARG(poly >= 0 && poly < win, "skimi_smooth_savgol: poly = %d outside 0..win - 1 = %d", poly, win - 1);
    if (frames == 0 || joints == 0) return SKIMI_OK;
    SKIMI_CHECK_ARG(X && Y && X != Y && fir && (win == 1 || (first && last)), "skimi_smooth_savgol: NULL input, operator or output, or Y is X");
    const long S = 3 * joints;
    const dim3 grid((unsigned)cdiv(S, 64)), block(64);
    hipStream_t st = (hipStream_t)stream;
    switch (win) {      // the windows smooth_skeleton's default reaches get a kernel of their own
        case 3: hipLaunchKernelGGL(smooth_savgol_kernel<3>, grid, block, 0, st, X, (long)frames, S, win, fir, first, last, Y); break;
        case 5: hipLaunchKernelGGL(smooth_savgol_kernel<5>, grid, block, 0, st, X, (long)frames, S, win, fir, first, last, Y); break;
        case 7: hipLaunchKernelGGL(smooth_savgol_kernel<7>, grid, block, 0, st, X, (long)frames, S, win, fir, first, last, Y); break;
        case 9: hipLaunchKernelGGL(smooth_savgol_kernel<9>, grid, block, 0, st, X, (long)frames, S, win, fir, first, last, Y); break;
        default: hipLaunchKernelGGL(smooth_savgol_kernel<0>, grid, block, 0, st, X, (long)frames, S, win, fir, first, last, Y);
    }
    SKIMI_LAUNCH_CHECK();
    return SKIMI_OK;
}

}  // extern "C"
