// Camera calibration from the corners of a plane target (camera_calibration/main.py: cv2.calibrateCamera on chessboard
// corners; Zhang's start, then Levenberg-Marquardt over the intrinsics and every board's pose).  DESIGN §2 "Calibration";
// restated in tests/calibrate_restated.py.  All arithmetic is float64, built with -ffp-contract=off.
//
// A call is three launches on the stream: a copy kernel that lays the shared object points out once per board (the
// homography kernel reads a source array per group), bev.hip's homography fit on the V boards, shared by all groups, and
// calibrate_kernel: one workgroup of 512 threads per group, which runs the masks, the start, every iteration, the standard
// deviations and the final errors.  No host synchronisation, no allocation, no atomics, no traffic between workgroups.
//
// Mapping.  A wave takes the views w, w + 8, ..., a lane the corners l, l + 64, ... of its view.  Every sum over the
// corners of a view is a xor butterfly over the wave (reduce.h's wave_sum), chunks of 64 corners added in order; every sum
// over the views is one thread's, in view order, except the three scalars of a trial (cost, |d|^2, |x|^2), which wave 0
// adds lane-strided over the views and then by the butterfly.  So a sum depends only on (view, corner) indices and a group
// is bitwise what it is alone, inside a batch and on a rerun.  A view's record in the workspace (kRec doubles: its blocks of
// J^T J, its pose, trial pose and step, and its part of the Schur complement) is written and read by the threads of this
// workgroup only, between workgroup barriers.
//
// Rules (the numbers are the header's):
//  1 masks: corner used iff its object and image coordinates are finite; view used in group g iff use[g, v] != 0, >= 4
//    used corners and homography status 1; < 3 used views, or 2 corners < free + 6 views, fails the group.
//  2 start of the intrinsics: K0 / dist0, or cv2's initCameraMatrix2D on the homographies with the principal point at the
//    frame centre.  A non-finite or zero focal length, a non-finite principal point or coefficient fails the group.
//  3 start of each pose from K^-1 Hn, R = the nearest rotation (svd3.h).
//  4 residual: rule 2 of the lens block on (R (X, Y, 0) + t).xy / z, in pixels, minus the corner; cost = sum r^2.
//  5 free intrinsics additive, R <- Exp(w) R, t <- t + dt; a fixed intrinsic: identity row and column, zero right side.
//  6 (H + lam diag H) d = -g through the Schur complement on the views, LDL^T without pivoting; lam0 = 1e-3.
//  7 accept iff the trial cost is finite and <= c (1 + 1e-14): lam <- max(lam / 10, 1e-16); else lam <- 10 lam.
//  8 stop: accepted step with |d| <= 3e-8 (1 + |x|) (x: the free intrinsics and the used views' t), lam >= 1e30, or
//    max_evals cost evaluations.
//  9 std from the Schur complement at lam = 0, re-linearised at the stopping point.
// 10 outputs.
#include <math.h>

#include "camera_lm.h"
#include "common.h"
#include "reduce.h"
#include "rodrigues.h"
#include "svd3.h"

namespace skimi {
namespace {

constexpr int kThreads = 512, kWaves = kThreads / 64;
constexpr int kNI = 12;                      // fx fy cx cy k1 k2 p1 p2 k3 k4 k5 k6
constexpr int kMaxViews = 1024;              // the per-view flags live in LDS
constexpr int kMaxCorners = 4096;
constexpr double kTau = 3e-8;                // rule 8
constexpr double kLam0 = 1e-3, kLamMin = 1e-16, kLamMax = 1e30;
// a view's record in the workspace
constexpr int oA = 0, oGa = 78, oC = 90, oB = 162, oGb = 183, oCost = 189;   // the blocks of J^T J and J^T r, and sum r^2
constexpr int kSum = 91;                                                   // A, ga and the cost are summed over the views
constexpr int oPose = 190, oTrial = 202, oD = 214;                          // R t, the trial's R t, the step (w, dt)
constexpr int oE = 220, oY = 310, oZ = 382, oPiv = 388;                     // C B*^-1 C^T | C B*^-1 gb, B*^-1 C^T, B*^-1 gb, min pivot
constexpr int oTc = 389, oDn = 390, oTn = 391, kRec = 392;                  // the trial's cost, |d_v|^2, |t_v|^2
enum Phase { STOP = 0, STEP = 1, LINEARISE = 2 };

__device__ constexpr int p12(int i, int j) { return i * kNI - i * (i - 1) / 2 + (j - i); }   // i <= j

struct CalArgs {
    const double *obj, *img, *K0, *dist0, *Hn;
    const unsigned char* use;
    const int32_t* hstatus;
    double *K, *dist, *R, *t, *rvec, *err, *vstats, *rms, *cost0, *cost, *std, *ws;
    int32_t *n_evals, *n_views, *n_corners, *success;
    int V, n, free_mask, max_evals;
    double width, height;
};

struct State {
    double in[kNI], tr[kNI], da[kNI];        // the intrinsics, the trial's, the step
    double S[kNI * kNI], rhs[kNI], sum[kSum], inv[kNI][kNI];
    double c, c0, lam, dn2, xn2, t3[3];
    int evals, success, failed, next, first, nviews, ncorners, nfree, std_ok;
};

// rule 1's corner, or false
__device__ __forceinline__ bool load_corner(const CalArgs& a, int v, int i, double& X, double& Y, double& u, double& w) {
    X = Y = u = w = 0.0;
    if (i >= a.n) return false;
    X = a.obj[2 * i], Y = a.obj[2 * i + 1];
    const double* p = a.img + 2 * ((long)v * a.n + i);
    u = p[0], w = p[1];
    return is_fin(X) && is_fin(Y) && is_fin(u) && is_fin(w);
}

// rule 4 up to the distorted point
struct Lens {
    double q[3], z, x, y, r2, r4, r6, num, den, c, a, xd, yd;
};
__device__ __forceinline__ void project(const double* in, const double* R, const double* t, double X, double Y, Lens& L) {
    L.q[0] = R[0] * X + R[1] * Y;
    L.q[1] = R[3] * X + R[4] * Y;
    L.q[2] = R[6] * X + R[7] * Y;
    L.z = L.q[2] + t[2];
    L.x = (L.q[0] + t[0]) / L.z;
    L.y = (L.q[1] + t[1]) / L.z;
    L.r2 = L.x * L.x + L.y * L.y;
    L.r4 = L.r2 * L.r2;
    L.r6 = L.r4 * L.r2;
    L.num = 1.0 + in[4] * L.r2 + in[5] * L.r4 + in[8] * L.r6;
    L.den = 1.0 + in[9] * L.r2 + in[10] * L.r4 + in[11] * L.r6;
    L.a = (2.0 * L.x) * L.y;
    const double dx = in[6] * L.a + in[7] * (L.r2 + (2.0 * L.x) * L.x);
    const double dy = in[6] * (L.r2 + (2.0 * L.y) * L.y) + in[7] * L.a;
    L.c = L.num / L.den;
    L.xd = L.x * L.c + dx;
    L.yd = L.y * L.c + dy;
}
__device__ __forceinline__ void residual2(const double* in, const Lens& L, double u, double w, double* r) {
    r[0] = (in[0] * L.xd + in[2]) - u;
    r[1] = (in[1] * L.yd + in[3]) - w;
}

__device__ __forceinline__ void load_pose(const double* p, double* R, double* t) {
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = p[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = p[9 + k];
}

// One view's blocks at the current point: the wave's lanes take its corners.  take: the accepted trial pose moves into
// the pose first.
__device__ inline void linearise_view(const CalArgs& a, const State& s, double* rec, int v, bool take, int lane) {
    double R[9], t[3], in[kNI];
    load_pose(rec + (take ? oTrial : oPose), R, t);
    if (take && lane == 0) {
#pragma unroll
        for (int k = 0; k < 9; ++k) rec[oPose + k] = R[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) rec[oPose + 9 + k] = t[k];
    }
#pragma unroll
    for (int i = 0; i < kNI; ++i) in[i] = s.in[i];
    const int fm = a.free_mask;
    bool first = true;
    for (int base = 0; base < a.n; base += 64) {
        double X, Y, u, w, r[2], Ji[2][kNI], Jp[2][6];
        const bool used = load_corner(a, v, base + lane, X, Y, u, w);
        Lens L;
        project(in, R, t, X, Y, L);
        residual2(in, L, u, w, r);
        {
            const double fx = in[0], fy = in[1];
            const double nump = in[4] + 2.0 * in[5] * L.r2 + 3.0 * in[8] * L.r4;
            const double denp = in[9] + 2.0 * in[10] * L.r2 + 3.0 * in[11] * L.r4;
            const double cp = (nump * L.den - L.num * denp) / (L.den * L.den);
            const double xr = L.x / L.den, yr = L.y / L.den;
            Ji[0][0] = L.xd, Ji[0][1] = 0.0, Ji[0][2] = 1.0, Ji[0][3] = 0.0;
            Ji[1][0] = 0.0, Ji[1][1] = L.yd, Ji[1][2] = 0.0, Ji[1][3] = 1.0;
            Ji[0][4] = fx * (xr * L.r2), Ji[0][5] = fx * (xr * L.r4), Ji[0][8] = fx * (xr * L.r6);
            Ji[1][4] = fy * (yr * L.r2), Ji[1][5] = fy * (yr * L.r4), Ji[1][8] = fy * (yr * L.r6);
            Ji[0][6] = fx * L.a, Ji[0][7] = fx * (L.r2 + (2.0 * L.x) * L.x);
            Ji[1][6] = fy * (L.r2 + (2.0 * L.y) * L.y), Ji[1][7] = fy * L.a;
            Ji[0][9] = -fx * ((xr * L.c) * L.r2), Ji[0][10] = -fx * ((xr * L.c) * L.r4), Ji[0][11] = -fx * ((xr * L.c) * L.r6);
            Ji[1][9] = -fy * ((yr * L.c) * L.r2), Ji[1][10] = -fy * ((yr * L.c) * L.r4), Ji[1][11] = -fy * ((yr * L.c) * L.r6);
            // d (x_d, y_d) / d (x, y), then d r / d Xc = a, and J = [q x a, a] over (w, dt)
            const double off = (L.a * cp + 2.0 * in[6] * L.x) + 2.0 * in[7] * L.y;
            const double xx = ((L.c + (2.0 * L.x) * L.x * cp) + 2.0 * in[6] * L.y) + 6.0 * in[7] * L.x;
            const double yy = ((L.c + (2.0 * L.y) * L.y * cp) + 6.0 * in[6] * L.y) + 2.0 * in[7] * L.x;
            Jp[0][3] = fx * (xx / L.z), Jp[0][4] = fx * (off / L.z), Jp[0][5] = fx * (-(xx * L.x + off * L.y) / L.z);
            Jp[1][3] = fy * (off / L.z), Jp[1][4] = fy * (yy / L.z), Jp[1][5] = fy * (-(off * L.x + yy * L.y) / L.z);
            cross3(L.q, Jp[0] + 3, Jp[0]);
            cross3(L.q, Jp[1] + 3, Jp[1]);
        }
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            if (!used) r[c] = 0.0;
#pragma unroll
            for (int i = 0; i < kNI; ++i)
                if (!used || !((fm >> i) & 1)) Ji[c][i] = 0.0;
#pragma unroll
            for (int k = 0; k < 6; ++k)
                if (!used) Jp[c][k] = 0.0;
        }
        auto emit = [&](int k, double val) {
            const double sum = wave_sum(val);
            if (lane == 0) rec[k] = first ? sum : rec[k] + sum;
        };
#pragma unroll
        for (int i = 0; i < kNI; ++i) {
#pragma unroll
            for (int j = i; j < kNI; ++j) emit(oA + p12(i, j), Ji[0][i] * Ji[0][j] + Ji[1][i] * Ji[1][j]);
            emit(oGa + i, Ji[0][i] * r[0] + Ji[1][i] * r[1]);
#pragma unroll
            for (int k = 0; k < 6; ++k) emit(oC + 6 * i + k, Ji[0][i] * Jp[0][k] + Ji[1][i] * Jp[1][k]);
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) {
#pragma unroll
            for (int l = k; l < 6; ++l) emit(oB + packed(k, l), Jp[0][k] * Jp[0][l] + Jp[1][k] * Jp[1][l]);
            emit(oGb + k, Jp[0][k] * r[0] + Jp[1][k] * r[1]);
        }
        emit(oCost, r[0] * r[0] + r[1] * r[1]);
        first = false;
    }
}

// B* = B + lam diag B as L D L^T without pivoting, in registers: D on the diagonal of f, L below it
struct Ldl6 {
    double f[6][6], piv;
};
__device__ __forceinline__ void factor6(const double* B, double lam, Ldl6& F) {
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) F.f[i][j] = i == j ? B[packed(i, i)] + lam * B[packed(i, i)] : B[packed(j, i)];
    F.piv = 1.79769313486231570815e308;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double d = F.f[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) d -= F.f[j][k] * F.f[j][k] * F.f[k][k];
        F.f[j][j] = d;
        F.piv = d < F.piv || d != d ? d : F.piv;
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double e = F.f[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) e -= F.f[i][k] * F.f[j][k] * F.f[k][k];
            F.f[i][j] = e / d;
        }
    }
}
__device__ __forceinline__ void solve6(const Ldl6& F, const double* b, double* x) {
    double y[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double e = b[i];
#pragma unroll
        for (int k = 0; k < i; ++k) e -= F.f[i][k] * y[k];
        y[i] = e;
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) y[i] = y[i] / F.f[i][i];
#pragma unroll
    for (int i = 5; i >= 0; --i) {
        double e = y[i];
#pragma unroll
        for (int k = i + 1; k < 6; ++k) e -= F.f[k][i] * x[k];
        x[i] = e;
    }
}

// A view's part of the Schur complement at lam: lane i < 12 solves B* y_i = c_i (row i of C), lane 12 B* z = gb; slot
// e < 78 (a lane's slots: lane, lane + 64) then forms entry (i, j) of C B*^-1 C^T = c_i . y_j, slot 78 + i the right side's c_i . z
__device__ inline void schur_view(double* rec, double lam, int lane) {
    double B[21], b[6], y[6];
#pragma unroll
    for (int k = 0; k < 21; ++k) B[k] = rec[oB + k];
    Ldl6 F;
    factor6(B, lam, F);
    const double* bp = lane < kNI ? rec + oC + 6 * lane : rec + oGb;
#pragma unroll
    for (int k = 0; k < 6; ++k) b[k] = bp[k];
    solve6(F, b, y);
    // entry e of the packed upper triangle -> (i, j); the 90 entries take two rounds of the wave
#pragma unroll
    for (int round = 0; round < 2; ++round) {
        const int slot = lane + 64 * round;
        int i = 0, j = kNI, e = slot;
        if (slot < 78) {
            while (e >= kNI - i) e -= kNI - i, ++i;
            j = i + e;
        } else if (slot < 90) {
            i = slot - 78;
        }
        const double* ci = rec + oC + 6 * i;
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const double yj = __shfl(y[k], j, 64);
            acc += ci[k] * yj;
        }
        if (slot < 90) rec[oE + slot] = acc;
    }
    if (lane < kNI) {
#pragma unroll
        for (int k = 0; k < 6; ++k) rec[oY + 6 * lane + k] = y[k];
    } else if (lane == kNI) {
#pragma unroll
        for (int k = 0; k < 6; ++k) rec[oZ + k] = y[k];
        rec[oPiv] = F.piv;
    }
}

// the reduced system of the intrinsics in s.S (both triangles) and s.rhs: threads e < 90, the views in order
__device__ inline void assemble(const CalArgs& a, State& s, const double* grec, const unsigned char* vused, double lam, int tid) {
    if (tid >= 90) return;
    double acc = 0.0;
    for (int v = 0; v < a.V; ++v)
        if (vused[v]) acc += grec[(long)v * kRec + oE + tid];
    if (tid < 78) {
        int i = 0, e = tid;
        while (e >= kNI - i) e -= kNI - i, ++i;
        const int j = i + e;
        const double A = s.sum[oA + tid];
        double val = (i == j ? A + lam * A : A) - acc;
        if (!((a.free_mask >> i) & 1) || !((a.free_mask >> j) & 1)) val = i == j ? 1.0 : 0.0;
        s.S[i * kNI + j] = s.S[j * kNI + i] = val;
    } else {
        const int i = tid - 78;
        s.rhs[i] = ((a.free_mask >> i) & 1) ? -s.sum[oGa + i] + acc : 0.0;
    }
}

// thread 0: s.S = L D L^T in place without pivoting; returns the smallest pivot
__device__ inline double factor12(double* S) {
    double piv = 1.79769313486231570815e308;
    for (int j = 0; j < kNI; ++j) {
        double d = S[j * kNI + j];
        for (int k = 0; k < j; ++k) d -= S[j * kNI + k] * S[j * kNI + k] * S[k * kNI + k];
        S[j * kNI + j] = d;
        piv = d < piv || d != d ? d : piv;
        for (int i = j + 1; i < kNI; ++i) {
            double e = S[i * kNI + j];
            for (int k = 0; k < j; ++k) e -= S[i * kNI + k] * S[j * kNI + k] * S[k * kNI + k];
            S[i * kNI + j] = e / d;
        }
    }
    return piv;
}
__device__ inline void solve12(const double* S, double* y) {
    for (int i = 0; i < kNI; ++i) {
        double e = y[i];
        for (int k = 0; k < i; ++k) e -= S[i * kNI + k] * y[k];
        y[i] = e;
    }
    for (int i = 0; i < kNI; ++i) y[i] = y[i] / S[i * kNI + i];
    for (int i = kNI - 1; i >= 0; --i) {
        double e = y[i];
        for (int k = i + 1; k < kNI; ++k) e -= S[k * kNI + i] * y[k];
        y[i] = e;
    }
}

// cv2.Rodrigues(R) -> rvec: a = the axial vector of (R - R^T) / 2 = sin(th) n, c = (tr R - 1) / 2, th = atan2(|a|, c)
__device__ inline void log_so3(const double* R, double* w) {
    const double a[3] = {0.5 * (R[7] - R[5]), 0.5 * (R[2] - R[6]), 0.5 * (R[3] - R[1])};
    const double sn = norm3(a[0], a[1], a[2]);
    const double c = fmin(fmax(0.5 * (((R[0] + R[4]) + R[8]) - 1.0), -1.0), 1.0);
    const double th = atan2(sn, c);
    if (c > -0.99) {
        const double f = sn < 1e-5 ? 1.0 + th * th / 6.0 : th / sn;
#pragma unroll
        for (int k = 0; k < 3; ++k) w[k] = f * a[k];
        return;
    }
    // near pi: n from the symmetric part, n n^T = ((R + R^T) / 2 - c I) / (1 - c), its sign from a
    const int k = R[0] >= R[4] && R[0] >= R[8] ? 0 : R[4] >= R[8] ? 1 : 2;
    const double dk = k == 0 ? R[0] : k == 1 ? R[4] : R[8];
    const double nk = sqrt(fmax((dk - c) / (1.0 - c), 0.0)), den = (1.0 - c) * nk;
    const double s01 = 0.5 * (R[1] + R[3]) / den, s02 = 0.5 * (R[2] + R[6]) / den, s12 = 0.5 * (R[5] + R[7]) / den;
    const double nv[3] = {k == 0 ? nk : k == 1 ? s01 : s02, k == 0 ? s01 : k == 1 ? nk : s12, k == 0 ? s02 : k == 1 ? s12 : nk};
    const double sg = dot3(nv, a) < 0.0 ? -1.0 : 1.0;
#pragma unroll
    for (int j = 0; j < 3; ++j) w[j] = sg * th * nv[j];
}

__global__ __launch_bounds__(64) void replicate_obj_kernel(const double* __restrict__ obj, double* __restrict__ out, int n2) {
    double* o = out + (long)blockIdx.x * n2;
    for (int i = threadIdx.x; i < n2; i += 64) o[i] = obj[i];
}

__global__ __launch_bounds__(kThreads) void calibrate_kernel(CalArgs a) {
    __shared__ State s;
    __shared__ unsigned char vused[kMaxViews];
    __shared__ int ncorn[kMaxViews];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long g = blockIdx.x;
    const int V = a.V, n = a.n;
    double* grec = a.ws + g * V * kRec;
    const double nan = qnan();

    // ---- rule 1 ----
    for (int v = wave; v < V; v += kWaves) {
        int cnt = 0;
        for (int base = 0; base < n; base += 64) {
            double X, Y, u, w;
            cnt += load_corner(a, v, base + lane, X, Y, u, w) ? 1 : 0;
        }
        cnt = wave_sum(cnt);
        if (lane == 0) {
            const bool on = !a.use || a.use[g * V + v] != 0;
            ncorn[v] = cnt;
            vused[v] = on && cnt >= 4 && a.hstatus[v] == 1 ? 1 : 0;
        }
    }
    __syncthreads();
    if (tid == 0) {
        int nv = 0, nc = 0, nf = 0;
        for (int v = 0; v < V; ++v)
            if (vused[v]) nv += 1, nc += ncorn[v];
        for (int i = 0; i < kNI; ++i) nf += (a.free_mask >> i) & 1;
        s.nviews = nv, s.ncorners = nc, s.nfree = nf;
        bool failed = nv < 3 || 2 * nc < nf + 6 * nv;
        // ---- rule 2 ----
        for (int i = 0; i < kNI; ++i) s.in[i] = 0.0;
        if (a.dist0)
            for (int i = 0; i < 8; ++i) s.in[4 + i] = a.dist0[g * 12 + i];
        if (a.K0) {
            const double* K = a.K0 + g * 9;
            s.in[0] = K[0], s.in[1] = K[4], s.in[2] = K[2], s.in[3] = K[5];
        } else if (!failed) {
            const double cx = (a.width - 1.0) / 2.0, cy = (a.height - 1.0) / 2.0;
            double n00 = 0.0, n01 = 0.0, n11 = 0.0, r0 = 0.0, r1 = 0.0;
            for (int v = 0; v < V; ++v) {
                if (!vused[v]) continue;
                const double* H = a.Hn + 9 * v;
                double h[3] = {H[0] - cx * H[6], H[3] - cy * H[6], H[6]}, w[3] = {H[1] - cx * H[7], H[4] - cy * H[7], H[7]};
                double d1[3], d2[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) d1[k] = (h[k] + w[k]) / 2.0, d2[k] = (h[k] - w[k]) / 2.0;
                const double nh = norm3(h[0], h[1], h[2]), nw = norm3(w[0], w[1], w[2]);
                const double n1 = norm3(d1[0], d1[1], d1[2]), n2 = norm3(d2[0], d2[1], d2[2]);
#pragma unroll
                for (int k = 0; k < 3; ++k) h[k] = h[k] / nh, w[k] = w[k] / nw, d1[k] = d1[k] / n1, d2[k] = d2[k] / n2;
                const double rows[2][3] = {{h[0] * w[0], h[1] * w[1], -(h[2] * w[2])}, {d1[0] * d2[0], d1[1] * d2[1], -(d1[2] * d2[2])}};
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    n00 += rows[k][0] * rows[k][0];
                    n01 += rows[k][0] * rows[k][1];
                    n11 += rows[k][1] * rows[k][1];
                    r0 += rows[k][0] * rows[k][2];
                    r1 += rows[k][1] * rows[k][2];
                }
            }
            const double det = n00 * n11 - n01 * n01;
            const double fa = (n11 * r0 - n01 * r1) / det, fb = (n00 * r1 - n01 * r0) / det;
            s.in[0] = sqrt(fabs(1.0 / fa));
            s.in[1] = sqrt(fabs(1.0 / fb));
            s.in[2] = cx, s.in[3] = cy;
        }
        for (int i = 0; i < kNI; ++i) failed = failed || !is_fin(s.in[i]);
        failed = failed || s.in[0] == 0.0 || s.in[1] == 0.0;
        s.failed = failed ? 1 : 0;
        s.evals = 0, s.success = 0, s.first = 1, s.std_ok = 0;
        s.c = s.c0 = nan;
        s.lam = kLam0;
        s.dn2 = s.xn2 = 0.0;
    }
    __syncthreads();
    bool failed = s.failed != 0;

    if (!failed) {
        // ---- rule 3: a thread per view ----
        for (int v = tid; v < V; v += kThreads) {
            if (!vused[v]) continue;
            const double* H = a.Hn + 9 * v;
            double M[9];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                M[c] = (H[c] - s.in[2] * H[6 + c]) / s.in[0];
                M[3 + c] = (H[3 + c] - s.in[3] * H[6 + c]) / s.in[1];
                M[6 + c] = H[6 + c];
            }
            const bool neg = M[8] < 0.0;
#pragma unroll
            for (int k = 0; k < 9; ++k) M[k] = neg ? -M[k] : M[k];
            const double sc = 1.0 / norm3(M[0], M[3], M[6]);
            const double r1[3] = {sc * M[0], sc * M[3], sc * M[6]}, r2[3] = {sc * M[1], sc * M[4], sc * M[7]};
            double r3[3], Q[9], R[9], ssum;
            cross3(r1, r2, r3);
#pragma unroll
            for (int k = 0; k < 3; ++k) Q[3 * k] = r1[k], Q[3 * k + 1] = r2[k], Q[3 * k + 2] = r3[k];
            polar3(Q, R, ssum);
            double* rec = grec + (long)v * kRec;
#pragma unroll
            for (int k = 0; k < 9; ++k) rec[oPose + k] = R[k];
#pragma unroll
            for (int k = 0; k < 3; ++k) rec[oPose + 9 + k] = sc * M[3 * k + 2];
        }
        __syncthreads();

        // ---- rules 4 to 8 ----
        int phase = LINEARISE;
        bool take = false;
        while (phase != STOP) {
            if (phase == LINEARISE) {
                for (int v = wave; v < V; v += kWaves)
                    if (vused[v]) linearise_view(a, s, grec + (long)v * kRec, v, take, lane);
                take = true;
                __syncthreads();
                if (tid < kSum) {
                    double acc = 0.0;
                    const int k = tid < 90 ? tid : oCost;
                    for (int v = 0; v < V; ++v)
                        if (vused[v]) acc += grec[(long)v * kRec + k];
                    s.sum[tid] = acc;
                }
                __syncthreads();
                if (tid == 0) {
                    s.c = s.sum[90];
                    bool ok = is_fin(s.c);
                    int next = STEP;
                    if (s.first) {
                        s.first = 0;
                        s.c0 = s.c;
                        s.evals = 1;
                        if (!ok) s.failed = 1, next = STOP;
                    } else if (!ok) {
                        next = STOP;
                    } else if (sqrt(s.dn2) <= kTau * (1.0 + sqrt(s.xn2))) {
                        s.success = 1;
                        next = STOP;
                    }
                    if (next == STEP && s.evals >= a.max_evals) next = STOP;
                    s.next = next;
                }
            } else {
                const double lam = s.lam;
                for (int v = wave; v < V; v += kWaves)
                    if (vused[v]) schur_view(grec + (long)v * kRec, lam, lane);
                __syncthreads();
                assemble(a, s, grec, vused, lam, tid);
                __syncthreads();
                if (tid == 0) {
                    factor12(s.S);
                    solve12(s.S, s.rhs);
                    for (int i = 0; i < kNI; ++i) {
                        s.da[i] = s.rhs[i];
                        s.tr[i] = ((a.free_mask >> i) & 1) ? s.in[i] + s.da[i] : s.in[i];
                    }
                    s.evals = s.evals + 1;
                }
                __syncthreads();
                // every view's step d_v = -(z + Y^T da), its trial pose, |d_v|^2 and |t|^2: a thread per view
                for (int v = tid; v < V; v += kThreads) {
                    if (!vused[v]) continue;
                    double* rec = grec + (long)v * kRec;
                    double d[6], R[9], t[3], R1[9], dn = 0.0, tn = 0.0;
#pragma unroll
                    for (int k = 0; k < 6; ++k) {
                        double e = rec[oZ + k];
                        for (int i = 0; i < kNI; ++i) e += rec[oY + 6 * i + k] * s.da[i];
                        d[k] = -e;
                        dn += d[k] * d[k];
                        rec[oD + k] = d[k];
                    }
                    load_pose(rec + oPose, R, t);
                    Rot r;
                    rodrigues(d, r);
                    rotate(r, R, R1);
#pragma unroll
                    for (int k = 0; k < 9; ++k) rec[oTrial + k] = R1[k];
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        const double tk = t[k] + d[3 + k];
                        rec[oTrial + 9 + k] = tk;
                        tn += tk * tk;
                    }
                    rec[oDn] = dn, rec[oTn] = tn;
                }
                __syncthreads();
                // the trial's cost, from the trial parameters
                for (int v = wave; v < V; v += kWaves) {
                    if (!vused[v]) continue;
                    double* rec = grec + (long)v * kRec;
                    double R[9], t[3], in[kNI], acc = 0.0;
                    load_pose(rec + oTrial, R, t);
#pragma unroll
                    for (int i = 0; i < kNI; ++i) in[i] = s.tr[i];
                    for (int base = 0; base < n; base += 64) {
                        double X, Y, u, w, r[2];
                        const bool used = load_corner(a, v, base + lane, X, Y, u, w);
                        Lens L;
                        project(in, R, t, X, Y, L);
                        residual2(in, L, u, w, r);
                        acc += wave_sum(used ? r[0] * r[0] + r[1] * r[1] : 0.0);
                    }
                    if (lane == 0) rec[oTc] = acc;
                }
                __syncthreads();
                if (wave == 0) {
                    double t3[3] = {0.0, 0.0, 0.0};
                    for (int v = lane; v < V; v += 64)
                        if (vused[v]) {
                            const double* rec = grec + (long)v * kRec;
                            t3[0] += rec[oTc], t3[1] += rec[oDn], t3[2] += rec[oTn];
                        }
#pragma unroll
                    for (int k = 0; k < 3; ++k) t3[k] = wave_sum(t3[k]);
                    if (tid == 0) {
                        int next = STEP;
                        if (is_fin(t3[0]) && t3[0] <= s.c * (1.0 + 1e-14)) {
                            double dn2 = t3[1], xn2 = t3[2];
                            for (int i = 0; i < kNI; ++i)
                                if ((a.free_mask >> i) & 1) dn2 += s.da[i] * s.da[i], xn2 += s.tr[i] * s.tr[i];
                            for (int i = 0; i < kNI; ++i) s.in[i] = s.tr[i];
                            s.dn2 = dn2, s.xn2 = xn2;
                            s.lam = fmax(s.lam / 10.0, kLamMin);
                            next = LINEARISE;
                        } else {
                            s.lam = 10.0 * s.lam;
                            if (!(s.lam < kLamMax) || s.evals >= a.max_evals) next = STOP;
                        }
                        s.next = next;
                    }
                }
            }
            __syncthreads();
            phase = s.next;
        }
        failed = s.failed != 0;

        // ---- rule 9: the blocks are those of the stopping point ----
        if (!failed) {
            for (int v = wave; v < V; v += kWaves)
                if (vused[v]) schur_view(grec + (long)v * kRec, 0.0, lane);
            __syncthreads();
            assemble(a, s, grec, vused, 0.0, tid);
            __syncthreads();
            if (tid == 0) {
                double piv = factor12(s.S);
                for (int v = 0; v < V; ++v)
                    if (vused[v]) {
                        const double pv = grec[(long)v * kRec + oPiv];
                        piv = pv < piv || pv != pv ? pv : piv;
                    }
                s.std_ok = piv > 0.0 ? 1 : 0;
            }
            __syncthreads();
        }
    }

    // ---- rule 10 ----
    const int m = 2 * s.ncorners, p = s.nfree + 6 * s.nviews;
    if (tid < kNI) {
        double sd = nan;
        if (!failed && s.std_ok && ((a.free_mask >> tid) & 1) && m > p) {
            double* e = s.inv[tid];                // column tid of S0^-1
            for (int i = 0; i < kNI; ++i) e[i] = i == tid ? 1.0 : 0.0;
            solve12(s.S, e);
            sd = sqrt(e[tid] * s.c / (double)(m - p));
        }
        a.std[g * 12 + tid] = sd;
        a.dist[g * 12 + tid] = failed ? nan : tid < 8 ? s.in[4 + tid] : 0.0;
    }
    if (tid == 0) {
        double* K = a.K + g * 9;
        K[0] = s.in[0], K[1] = 0.0, K[2] = s.in[2], K[3] = 0.0, K[4] = s.in[1], K[5] = s.in[3], K[6] = 0.0, K[7] = 0.0, K[8] = 1.0;
        if (failed)
            for (int k = 0; k < 9; ++k) K[k] = nan;
        a.rms[g] = failed ? nan : sqrt(s.c / (double)s.ncorners);
        a.cost0[g] = failed ? nan : s.c0;
        a.cost[g] = failed ? nan : s.c;
        a.n_evals[g] = failed ? 0 : s.evals;
        a.n_views[g] = s.nviews;
        a.n_corners[g] = s.ncorners;
        a.success[g] = failed ? 0 : s.success;
    }
    for (int v = wave; v < V; v += kWaves) {
        const bool on = !failed && vused[v];
        const long pv = g * V + v;
        const double* rec = grec + (long)v * kRec;
        double R[9], t[3], in[kNI], sums[2] = {0.0, 0.0}, emax = 0.0;
        load_pose(rec + oPose, R, t);              // an unused view's record was never written: masked below
#pragma unroll
        for (int k = 0; k < 9; ++k) R[k] = on ? R[k] : nan;
#pragma unroll
        for (int k = 0; k < 3; ++k) t[k] = on ? t[k] : nan;
#pragma unroll
        for (int i = 0; i < kNI; ++i) in[i] = s.in[i];
        for (int base = 0; base < n; base += 64) {
            double X, Y, u, w, r[2], e = nan;
            const bool used = load_corner(a, v, base + lane, X, Y, u, w) && on;
            if (used) {
                Lens L;
                project(in, R, t, X, Y, L);
                residual2(in, L, u, w, r);
                e = sqrt(r[0] * r[0] + r[1] * r[1]);
            }
            if (base + lane < n) a.err[pv * n + base + lane] = e;
            sums[0] += wave_sum(used ? e : 0.0);
            sums[1] += wave_sum(used ? e * e : 0.0);
            double mx = used ? e : 0.0;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) mx = max_nan(mx, __shfl_xor(mx, o, 64));
            emax = max_nan(emax, mx);
        }
        if (lane == 0) {
            const double cnt = (double)ncorn[v];
            double w[3] = {nan, nan, nan};
            if (on) log_so3(R, w);
#pragma unroll
            for (int k = 0; k < 9; ++k) a.R[pv * 9 + k] = R[k];
#pragma unroll
            for (int k = 0; k < 3; ++k) a.t[pv * 3 + k] = t[k], a.rvec[pv * 3 + k] = w[k];
            a.vstats[pv * 3] = on ? sums[0] / cnt : nan;
            a.vstats[pv * 3 + 1] = on ? sqrt(sums[1] / cnt) : nan;
            a.vstats[pv * 3 + 2] = on ? emax : nan;
        }
    }
}

// the workspace: the object points once per board and the homography fit's outputs, then a record per (group, view)
struct WsLayout {
    size_t obj, H, Hinv, Hn, herr, hstats, hstatus, rec, bytes;
};
__host__ inline WsLayout ws_layout(int64_t G, int64_t V, int64_t n) {
    WsLayout w;
    size_t o = 0;
    auto take = [&](size_t count) {
        const size_t at = o;
        o += (count * sizeof(double) + 255) / 256 * 256;
        return at;
    };
    w.obj = take((size_t)V * n * 2);
    w.H = take((size_t)V * 9);
    w.Hinv = take((size_t)V * 9);
    w.Hn = take((size_t)V * 9);
    w.herr = take((size_t)V * n);
    w.hstats = take((size_t)V * 4);
    w.hstatus = take((size_t)V);
    w.rec = take((size_t)G * V * kRec);
    w.bytes = o;
    return w;
}
__host__ inline bool sizes_ok(int64_t G, int64_t V, int64_t n) {
    return G >= 1 && G <= 65535 * 16 && V >= 1 && V <= kMaxViews && n >= 4 && n <= kMaxCorners;
}

}  // namespace
}  // namespace skimi

using namespace skimi;

extern "C" {

size_t skimi_calibrate_workspace_bytes(int64_t G, int32_t V, int32_t n) {
    if (!sizes_ok(G, V, n)) return 0;
    return ws_layout(G, V, n).bytes;
}

int skimi_calibrate_camera(const double* obj, const double* img, const uint8_t* use, const double* K0, const double* dist0, int64_t G,
                           int32_t V, int32_t n, int32_t width, int32_t height, int32_t free_mask, int32_t max_evals, double* K,
                           double* dist, double* R, double* t, double* rvec, double* err, double* view_stats, double* rms,
                           double* cost0, double* cost, double* std, int32_t* n_evals, int32_t* n_views, int32_t* n_corners,
                           int32_t* success, void* ws, size_t ws_bytes, void* stream) {
    SKIMI_CHECK_ARG(obj && img, "skimi_calibrate_camera: NULL input");
    SKIMI_CHECK_ARG(K && dist && R && t && rvec && err && view_stats && rms && cost0 && cost && std && n_evals && n_views && n_corners &&
                        success,
                    "skimi_calibrate_camera: NULL output");
    SKIMI_CHECK_ARG(G >= 1 && G <= 65535 * 16, "skimi_calibrate_camera: G = %lld outside 1 .. %d", (long long)G, 65535 * 16);
    SKIMI_CHECK_ARG(V >= 1 && V <= kMaxViews, "skimi_calibrate_camera: %d views outside 1 .. %d", V, kMaxViews);
    SKIMI_CHECK_ARG(n >= 4 && n <= kMaxCorners, "skimi_calibrate_camera: %d corners a board outside 4 .. %d", n, kMaxCorners);
    SKIMI_CHECK_ARG(width >= 1 && height >= 1, "skimi_calibrate_camera: image size %d x %d", width, height);
    SKIMI_CHECK_ARG(free_mask >= 0 && free_mask < (1 << kNI), "skimi_calibrate_camera: free_mask = %d outside 12 bits", free_mask);
    SKIMI_CHECK_ARG(max_evals >= 1, "skimi_calibrate_camera: max_evals = %d < 1", max_evals);
    const WsLayout w = ws_layout(G, V, n);
    SKIMI_CHECK_ARG(ws && ws_bytes >= w.bytes, "skimi_calibrate_camera: workspace of %zu bytes, need %zu", ws_bytes, w.bytes);
    SKIMI_CHECK_ARG(((uintptr_t)ws & 7) == 0, "skimi_calibrate_camera: workspace not 8-byte aligned");
    char* base = (char*)ws;
    double* obj_rep = (double*)(base + w.obj);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(replicate_obj_kernel, dim3((unsigned)V), dim3(64), 0, st, obj, obj_rep, 2 * n);
    SKIMI_LAUNCH_CHECK();
    const int rc = skimi_homography_fit(obj_rep, img, nullptr, V, n, (double*)(base + w.H), (double*)(base + w.Hinv),
                                        (double*)(base + w.Hn), (double*)(base + w.herr), (double*)(base + w.hstats),
                                        (int32_t*)(base + w.hstatus), stream);
    if (rc != SKIMI_OK) return rc;
    CalArgs a{};
    a.obj = obj, a.img = img, a.K0 = K0, a.dist0 = dist0, a.Hn = (const double*)(base + w.Hn);
    a.use = use, a.hstatus = (const int32_t*)(base + w.hstatus);
    a.K = K, a.dist = dist, a.R = R, a.t = t, a.rvec = rvec, a.err = err, a.vstats = view_stats, a.rms = rms, a.cost0 = cost0;
    a.cost = cost, a.std = std, a.ws = (double*)(base + w.rec);
    a.n_evals = n_evals, a.n_views = n_views, a.n_corners = n_corners, a.success = success;
    a.V = V, a.n = n, a.free_mask = free_mask, a.max_evals = max_evals;
    a.width = (double)width, a.height = (double)height;
    hipLaunchKernelGGL(calibrate_kernel, dim3((unsigned)G), dim3(kThreads), 0, st, a);
    SKIMI_LAUNCH_CHECK();
    return SKIMI_OK;
}

}  // extern "C"
