// Pose evaluation of clips of 3D joints: the MPJPE protocols of VideoPose3D/common/loss.py with the per-joint tables of
// metrics/unity_data_compare.py (skimi_pose_errors), and the ground-truth-free quality figures of VideoPose3D/fuse/
// fuse_eval.py and metrics/true_data_compare.py (skimi_clip_quality).  tests/evaluate_restated.py is the restatement;
// rules: include/skimi.h and DESIGN §2 "Evaluation".
//
// skimi_pose_errors, three launches for all clips:
//  (a) pe_frame_kernel: one wave per (clip, frame), lanes over joints (two per lane above 64).  Every sum is a per-lane
//      sum followed by a fixed xor butterfly, so all lanes hold the same bits and the 3 x 3 Procrustes problem (svd3.h, the
//      decomposition of the fusion) runs uniformly across the wave.
//  (b) pe_clip_kernel: one workgroup per clip -> the four clip means and the counts.  A thread sums the samples tid, tid +
//      256, .. of the clip's own index space (length x joints, or length), then the waves' butterflies, then the four wave
//      totals in order: the order is a function of the clip's length alone.
//  (c) pe_joint_kernel: one wave per (clip, table, joint) -> mean, two-pass std, exact median, n of the finite samples.
// skimi_clip_quality, one launch: one workgroup per clip.  The interpolated copy of the clip and the two difference-norm
// series of the percentiles (five of frames x joints doubles) live in LDS or in a workspace; the code is the same, only
// the pointer differs.
// Order statistics are exact: a bitwise binary search over the order-preserving 64-bit key of a double, one counting pass
// per bit (integer counts: exact in any order); both ranks of a median or percentile are found in the same passes.
// All arithmetic is float64 and the file is compiled without FMA contraction.  No floating-point atomics.
#include <math.h>

#include "common.h"
#include "fp64_util.h"
#include "reduce.h"
#include "svd3.h"

namespace skimi {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxJoints = SKIMI_EVAL_MAX_JOINTS;
constexpr int kMaxEdges = SKIMI_EVAL_MAX_EDGES;
constexpr int kMaxPairs = SKIMI_EVAL_MAX_PAIRS;
constexpr long kMaxElems = 1L << 40;

__device__ inline int clip_len(const int32_t* lengths, long b, long T) {
    return lengths ? (int)min(max((long)lengths[b], 0L), T) : (int)T;
}

// the sum over the workgroup: the waves' butterflies, then the four wave totals in order.  sh: kWaves values in LDS.
__device__ inline double block_sum(double x, double* sh) {
    x = wave_sum(x);
    __syncthreads();                                   // the previous call's readers are done
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = x;
    __syncthreads();
    return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}
__device__ inline int block_isum(int x, int* sh) {
    x = wave_sum(x);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = x;
    __syncthreads();
    return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// ---- skimi_pose_errors -------------------------------------------------------------------------------------------
struct PeArgs {
    const double *pred, *target;
    const int32_t* lengths;
    double *err, *p_err, *vel_err, *mpjpe_f, *n_mpjpe_f, *p_mpjpe_f, *aligned, *p_R, *p_scale, *p_t, *metrics, *joint_stats;
    int32_t *n_valid_f, *p_status, *counts, *joint_n;
    long B, T;
    int J, zero_root;
};

// (a) one wave per (clip, frame)
__global__ __launch_bounds__(kThreads) void pe_frame_kernel(PeArgs a) {
    const long f = (long)blockIdx.x * kWaves + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (f >= a.B * a.T) return;                        // uniform across the wave
    const long b = f / a.T;
    const int t = (int)(f - b * a.T), J = a.J;
    const double nan = qnan();
    double e[2], pe[2], ve[2], al[2][3];
    double mf = nan, nf = nan, pf = nan, sc = nan, R[9], tv[3];
    int nvalid = 0, status = 0;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        e[s] = pe[s] = ve[s] = nan;
        al[s][0] = al[s][1] = al[s][2] = nan;
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = nan;
    tv[0] = tv[1] = tv[2] = nan;

    if (t < clip_len(a.lengths, b, a.T)) {
        const double *P = a.pred + f * (long)J * 3, *G = a.target + f * (long)J * 3;
        double p[2][3], g[2][3];
        bool in[2], ok[2];
        double se = 0.0;
        int ce = 0, cv = 0;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int j = lane + 64 * s;
            in[s] = j < J;
            ok[s] = false;
#pragma unroll
            for (int c = 0; c < 3; ++c) p[s][c] = g[s][c] = 0.0;
            if (in[s]) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    p[s][c] = P[3 * j + c];
                    g[s][c] = j == a.zero_root ? 0.0 : G[3 * j + c];
                }
                ok[s] = fin3(p[s]) && fin3(g[s]);
                if (ok[s]) {
                    e[s] = norm3(p[s][0] - g[s][0], p[s][1] - g[s][1], p[s][2] - g[s][2]);
                    ++cv;
                    if (is_fin(e[s])) {
                        se += e[s];
                        ++ce;
                    }
                }
                if (t >= 1) {                          // the velocity error against the frame before
                    double pp[3], gp[3];
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        pp[c] = P[3 * j + c - (long)J * 3];
                        gp[c] = j == a.zero_root ? 0.0 : G[3 * j + c - (long)J * 3];
                    }
                    if (ok[s] && fin3(pp) && fin3(gp))
                        ve[s] = norm3((p[s][0] - pp[0]) - (g[s][0] - gp[0]), (p[s][1] - pp[1]) - (g[s][1] - gp[1]),
                                      (p[s][2] - pp[2]) - (g[s][2] - gp[2]));
                }
            }
        }
        se = wave_sum(se);
        ce = wave_sum(ce);
        nvalid = wave_sum(cv);
        if (ce > 0) mf = se / (double)ce;
        if (nvalid == J) {                             // a complete frame (uniform)
            const double dJ = (double)J;
            // N-MPJPE: the scale that matches the prediction to the target, then the mean distance
            double sgp = 0.0, spp = 0.0;
#pragma unroll
            for (int s = 0; s < 2; ++s)
                if (in[s]) {
                    sgp += g[s][0] * p[s][0] + g[s][1] * p[s][1] + g[s][2] * p[s][2];
                    spp += p[s][0] * p[s][0] + p[s][1] * p[s][1] + p[s][2] * p[s][2];
                }
            const double scale = (wave_sum(sgp) / dJ) / (wave_sum(spp) / dJ);
            double sn = 0.0;
#pragma unroll
            for (int s = 0; s < 2; ++s)
                if (in[s]) sn += norm3(scale * p[s][0] - g[s][0], scale * p[s][1] - g[s][1], scale * p[s][2] - g[s][2]);
            sn = wave_sum(sn) / dJ;
            if (is_fin(sn)) nf = sn;
            // Procrustes: centre, normalise, H = X0^T Y0, R = V U^T without reflection
            double muX[3], muY[3], x0[2][3], y0[2][3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                muX[c] = wave_sum(g[0][c] + g[1][c]) / dJ;      // joints outside the frame hold 0
                muY[c] = wave_sum(p[0][c] + p[1][c]) / dJ;
            }
            double sx = 0.0, sy = 0.0;
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    x0[s][c] = in[s] ? g[s][c] - muX[c] : 0.0;
                    y0[s][c] = in[s] ? p[s][c] - muY[c] : 0.0;
                    sx += x0[s][c] * x0[s][c];
                    sy += y0[s][c] * y0[s][c];
                }
            const double nX = sqrt(wave_sum(sx)), nY = sqrt(wave_sum(sy));
            double H[9];
            bool fin = nX > 0.0 && nY > 0.0;              // a pose without extent has no alignment
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int c = 0; c < 3; ++c) x0[s][c] /= nX, y0[s][c] /= nY;
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    double h = 0.0;
#pragma unroll
                    for (int s = 0; s < 2; ++s)
                        if (in[s]) h += x0[s][r] * y0[s][c];
                    H[3 * r + c] = wave_sum(h);
                    fin = fin && is_fin(H[3 * r + c]);
                }
            if (fin) {
                double Q[9], ssum, smin, sign;
                polar3_signed(H, Q, ssum, smin, sign);
                const double tr = sign < 0.0 ? ssum - 2.0 * smin : ssum;
                const double as = tr * nX / nY;
                double Rm[9], tt[3];
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int c = 0; c < 3; ++c) Rm[3 * r + c] = Q[3 * c + r];
#pragma unroll
                for (int c = 0; c < 3; ++c) tt[c] = muX[c] - as * (muY[0] * Rm[c] + muY[1] * Rm[3 + c] + muY[2] * Rm[6 + c]);
                double sp = 0.0, q[2][3], d[2];
#pragma unroll
                for (int s = 0; s < 2; ++s) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) q[s][c] = as * (p[s][0] * Rm[c] + p[s][1] * Rm[3 + c] + p[s][2] * Rm[6 + c]) + tt[c];
                    d[s] = norm3(q[s][0] - g[s][0], q[s][1] - g[s][1], q[s][2] - g[s][2]);
                    if (in[s]) sp += d[s];
                }
                sp = wave_sum(sp) / dJ;
                bool good = is_fin(sp) && is_fin(as) && fin3(tt);
#pragma unroll
                for (int k = 0; k < 9; ++k) good = good && is_fin(Rm[k]);
                if (good) {
                    status = 1;
                    pf = sp, sc = as;
#pragma unroll
                    for (int k = 0; k < 9; ++k) R[k] = Rm[k];
#pragma unroll
                    for (int s = 0; s < 2; ++s) {
                        pe[s] = d[s];
#pragma unroll
                        for (int c = 0; c < 3; ++c) al[s][c] = q[s][c];
                    }
#pragma unroll
                    for (int c = 0; c < 3; ++c) tv[c] = tt[c];
                }
            }
        }
    }
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int j = lane + 64 * s;
        if (j < J) {
            const long o = f * J + j;
            a.err[o] = e[s];
            a.p_err[o] = pe[s];
            a.vel_err[o] = ve[s];
            if (a.aligned) {
#pragma unroll
                for (int c = 0; c < 3; ++c) a.aligned[3 * o + c] = al[s][c];
            }
        }
    }
    if (lane == 0) {
        a.mpjpe_f[f] = mf;
        a.n_mpjpe_f[f] = nf;
        a.p_mpjpe_f[f] = pf;
        a.n_valid_f[f] = nvalid;
        a.p_status[f] = status;
        if (a.p_scale) a.p_scale[f] = sc;
        if (a.p_R) {
#pragma unroll
            for (int k = 0; k < 9; ++k) a.p_R[9 * f + k] = R[k];
        }
        if (a.p_t) {
#pragma unroll
            for (int c = 0; c < 3; ++c) a.p_t[3 * f + c] = tv[c];
        }
    }
}

// (b) one workgroup per clip: the mean of the finite samples of x[0 .. m), and their number
__device__ inline double clip_mean(const double* x, long m, double* shd, int* shi, int& count) {
    double s = 0.0;
    int c = 0;
    for (long i = threadIdx.x; i < m; i += kThreads) {
        const double v = x[i];
        if (is_fin(v)) {
            s += v;
            ++c;
        }
    }
    s = block_sum(s, shd);
    count = block_isum(c, shi);
    return count > 0 ? s / (double)count : qnan();
}

__global__ __launch_bounds__(kThreads) void pe_clip_kernel(PeArgs a) {
    __shared__ double shd[kWaves];
    __shared__ int shi[kWaves];
    const long b = blockIdx.x, base = b * a.T;
    const int n = clip_len(a.lengths, b, a.T);
    int n_err, n_vel, n_p, n_n, c = 0;
    const double m1 = clip_mean(a.err + base * a.J, (long)n * a.J, shd, shi, n_err);
    const double mv = clip_mean(a.vel_err + base * a.J, (long)n * a.J, shd, shi, n_vel);
    const double m2 = clip_mean(a.p_mpjpe_f + base, n, shd, shi, n_p);
    const double m3 = clip_mean(a.n_mpjpe_f + base, n, shd, shi, n_n);
    for (int i = threadIdx.x; i < n; i += kThreads) c += a.n_valid_f[base + i] == a.J;
    c = block_isum(c, shi);
    if (threadIdx.x == 0) {
        double* o = a.metrics + b * 4;
        o[SKIMI_PE_MPJPE] = m1, o[SKIMI_PE_P_MPJPE] = m2, o[SKIMI_PE_N_MPJPE] = m3, o[SKIMI_PE_MPJVE] = mv;
        a.counts[3 * b] = n_err, a.counts[3 * b + 1] = c, a.counts[3 * b + 2] = n_vel;
    }
}

// (c) one wave per (clip, table, joint): table 0 = err, 1 = p_err
__global__ __launch_bounds__(kThreads) void pe_joint_kernel(PeArgs a) {
    const long w = (long)blockIdx.x * kWaves + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63, J = a.J;
    if (w >= a.B * 2 * J) return;
    const long r = w / J;                              // (clip, table)
    const int j = (int)(w - r * J);
    const long b = r >> 1;
    const int n = clip_len(a.lengths, b, a.T);
    const double* x = ((r & 1) ? a.p_err : a.err) + b * a.T * J + j;
    double mean = qnan(), sd = qnan(), med = qnan();
    double s = 0.0;
    int cnt = 0;
    for (int i = lane; i < n; i += 64) {
        const double v = x[(long)i * J];
        if (is_fin(v)) {
            s += v;
            ++cnt;
        }
    }
    s = wave_sum(s);
    cnt = wave_sum(cnt);
    if (cnt > 0) {
        mean = s / (double)cnt;
        double ss = 0.0;
        for (int i = lane; i < n; i += 64) {
            const double v = x[(long)i * J];
            if (is_fin(v)) ss += (v - mean) * (v - mean);
        }
        sd = sqrt(wave_sum(ss) / (double)cnt);
        // the two middle order statistics (the same one for an odd count)
        unsigned long long p0, p1;
        wave_select2((unsigned)(cnt - 1) / 2, (unsigned)cnt / 2, [&](auto&& f) {
            for (int i = lane; i < n; i += 64) {
                const double v = x[(long)i * J];
                if (is_fin(v)) f(key64(v));
            }
        }, p0, p1);
        med = (unkey64(p0) + unkey64(p1)) / 2.0;
    }
    if (lane == 0) {
        double* o = a.joint_stats + w * 3;
        o[0] = mean, o[1] = sd, o[2] = med;
        a.joint_n[w] = cnt;
    }
}

// ---- skimi_clip_quality ------------------------------------------------------------------------------------------
struct CqArgs {
    const double* X;
    const int32_t* lengths;
    double *ws, *scalars, *cv_edge, *bone_len;
    long B, T, stride;
    int J, E, EL, ER, P;
    uint8_t edges[kMaxEdges][2], ledges[kMaxEdges][2], redges[kMaxEdges][2], pairs[kMaxPairs][2];
};

// the length of a bone in one frame; NaN unless both endpoints are finite
__device__ inline double bone(const double* frame, int ia, int ib) {
    const double *pa = frame + 3 * ia, *pb = frame + 3 * ib;
    if (!(fin3(pa) && fin3(pb))) return qnan();
    return norm3(pb[0] - pa[0], pb[1] - pa[1], pb[2] - pa[2]);
}

// nanmean of the bone lengths of an edge list over the clip's frames (count through `count`)
__device__ inline double bones_mean(const double* Xc, int n, int J, const uint8_t (*ed)[2], int E, double* shd, int* shi, int& count) {
    double s = 0.0;
    int c = 0;
    for (long i = threadIdx.x; i < (long)n * E; i += kThreads) {
        const int t = (int)(i / E), e = (int)(i - (long)t * E);
        const double L = bone(Xc + (long)t * J * 3, ed[e][0], ed[e][1]);
        if (L == L) {
            s += L;
            ++c;
        }
    }
    s = block_sum(s, shd);
    count = block_isum(c, shi);
    return count > 0 ? s / (double)count : qnan();
}

__global__ __launch_bounds__(kThreads) void clip_quality_kernel(CqArgs a) {
    extern __shared__ double lds[];
    __shared__ double shd[kWaves], sh_cv[kMaxEdges];
    __shared__ int shi[kWaves], sh_has[kMaxEdges];
    __shared__ unsigned sh_cnt[kWaves][4];
    const long b = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int J = a.J, E = a.E, n = clip_len(a.lengths, b, a.T);
    const double* Xc = a.X + b * a.T * J * 3;
    const double nan = qnan();
    double* out = a.scalars + b * SKIMI_CQ_SCALARS;

    // bone lengths: the optional output, then the pooled coefficient of variation (two passes)
    if (a.bone_len)
        for (long i = tid; i < a.T * E; i += kThreads) {
            const int t = (int)(i / E), e = (int)(i - (long)t * E);
            a.bone_len[b * a.T * E + i] = t < n ? bone(Xc + (long)t * J * 3, a.edges[e][0], a.edges[e][1]) : nan;
        }
    int cb;
    const double mb = bones_mean(Xc, n, J, a.edges, E, shd, shi, cb);
    double cv_pooled = nan;
    {
        double ss = 0.0;
        for (long i = tid; i < (long)n * E; i += kThreads) {
            const int t = (int)(i / E), e = (int)(i - (long)t * E);
            const double L = bone(Xc + (long)t * J * 3, a.edges[e][0], a.edges[e][1]);
            if (L == L) ss += (L - mb) * (L - mb);
        }
        ss = block_sum(ss, shd);
        if (cb > 0) cv_pooled = sqrt(ss / (double)cb) / (mb + 1e-9);
    }
    // per edge: one wave per edge, lanes over the frames
    for (int e = wave; e < E; e += kWaves) {
        const int ia = a.edges[e][0], ib = a.edges[e][1];
        double s = 0.0;
        int c = 0;
        for (int t = lane; t < n; t += 64) {
            const double L = bone(Xc + (long)t * J * 3, ia, ib);
            if (L == L) {
                s += L;
                ++c;
            }
        }
        s = wave_sum(s);
        c = wave_sum(c);
        double cv = nan;
        int has = 0;
        if (c > 0) {
            const double m = s / (double)c;
            double ss = 0.0;
            for (int t = lane; t < n; t += 64) {
                const double L = bone(Xc + (long)t * J * 3, ia, ib);
                if (L == L) ss += (L - m) * (L - m);
            }
            ss = wave_sum(ss);
            if (m > 1e-9) {
                cv = sqrt(ss / (double)c) / m;
                has = 1;
            }
        }
        if (lane == 0) {
            sh_cv[e] = cv, sh_has[e] = has;
            a.cv_edge[b * E + e] = cv;
        }
    }
    // left / right mean lengths
    int cl, cr;
    const double Lm = bones_mean(Xc, n, J, a.ledges, a.EL, shd, shi, cl);      // its barriers also publish sh_cv
    const double Rm = bones_mean(Xc, n, J, a.redges, a.ER, shd, shi, cr);
    const double lr_sym = fabs(Lm - Rm) / (0.5 * (Lm + Rm) + 1e-9);

    // speed and jerk: first and second differences where all three coordinates of the difference are finite
    double speed_mean = nan, jerk_mean = nan, speed_p95 = nan, accel_p95 = nan;
    if (n >= 3) {                                      // uniform
        double s = 0.0;
        int c = 0;
        for (long i = tid; i < (long)(n - 1) * J; i += kThreads) {
            const double* x = Xc + i * 3;
            const double d[3] = {x[3 * J] - x[0], x[3 * J + 1] - x[1], x[3 * J + 2] - x[2]};
            if (fin3(d)) {
                s += norm3(d[0], d[1], d[2]);
                ++c;
            }
        }
        s = block_sum(s, shd);
        c = block_isum(c, shi);
        if (c > 0) speed_mean = s / (double)c;
        s = 0.0, c = 0;
        for (long i = tid; i < (long)(n - 2) * J; i += kThreads) {
            const double* x = Xc + i * 3;
            double d[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) d[k] = (x[6 * J + k] - x[3 * J + k]) - (x[3 * J + k] - x[k]);
            if (fin3(d)) {
                s += norm3(d[0], d[1], d[2]);
                ++c;
            }
        }
        s = block_sum(s, shd);
        c = block_isum(c, shi);
        if (c > 0) jerk_mean = s / (double)c;

        // the percentiles: np.interp of every (joint, coordinate) series with at least 2 finite samples
        double* Xf = a.ws ? a.ws + b * a.stride : lds;
        double *V = Xf + a.T * J * 3, *A = V + a.T * J;
        const int S = 3 * J;
        for (int q = tid; q < S; q += kThreads) {      // one thread per series, sequential in time
            int cf = 0;
            for (int t = 0; t < n; ++t) cf += is_fin(Xc[(long)t * S + q]);
            if (cf < 2) {
                for (int t = 0; t < n; ++t) Xf[(long)t * S + q] = Xc[(long)t * S + q];
                continue;
            }
            int prev = -1;
            double yp = 0.0;
            for (int t = 0; t < n; ++t) {
                const double y = Xc[(long)t * S + q];
                if (!is_fin(y)) continue;
                if (prev < 0) {
                    for (int u = 0; u < t; ++u) Xf[(long)u * S + q] = y;          // the first value held
                } else {
                    const double slope = (y - yp) / (double)(t - prev);
                    for (int u = prev + 1; u < t; ++u) Xf[(long)u * S + q] = slope * (double)(u - prev) + yp;
                }
                Xf[(long)t * S + q] = y;
                prev = t, yp = y;
            }
            for (int u = prev + 1; u < n; ++u) Xf[(long)u * S + q] = yp;          // the last value held
        }
        __syncthreads();
        const unsigned mv = (unsigned)(n - 1) * (unsigned)J, ma = (unsigned)(n - 2) * (unsigned)J;
        int nv = 0, na = 0;
        for (unsigned i = tid; i < mv; i += kThreads) {
            const double* x = Xf + (long)i * 3;
            const double v = norm3(x[S] - x[0], x[S + 1] - x[1], x[S + 2] - x[2]);
            V[i] = v;
            nv += v != v;
            if (i < ma) {
                const double w = norm3((x[2 * S] - x[S]) - (x[S] - x[0]), (x[2 * S + 1] - x[S + 1]) - (x[S + 1] - x[1]),
                                       (x[2 * S + 2] - x[S + 2]) - (x[S + 2] - x[2]));
                A[i] = w;
                na += w != w;
            }
        }
        nv = block_isum(nv, shi);                       // its barriers also publish V and A
        na = block_isum(na, shi);
        // four selections in the same 64 passes: ranks i0, i1 of V and of A
        const PctPos pv = pct_pos(95.0, mv), pa = pct_pos(95.0, ma);
        unsigned kk[4] = {pv.i0, pv.i1, pa.i0, pa.i1};
        const double gv = pv.gamma, ga = pa.gamma;
        unsigned long long pre[4] = {0, 0, 0, 0};
        for (int bit = 63; bit >= 0; --bit) {
            unsigned c4[4] = {0, 0, 0, 0};
            for (unsigned i = tid; i < mv; i += kThreads) {
                const unsigned long long key = key64(V[i]);
                c4[0] += ((key ^ pre[0]) >> bit) == 0;
                c4[1] += ((key ^ pre[1]) >> bit) == 0;
                if (i < ma) {
                    const unsigned long long ka = key64(A[i]);
                    c4[2] += ((ka ^ pre[2]) >> bit) == 0;
                    c4[3] += ((ka ^ pre[3]) >> bit) == 0;
                }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) c4[k] = wave_sum(c4[k]);
            __syncthreads();
            if (lane == 0) {
#pragma unroll
                for (int k = 0; k < 4; ++k) sh_cnt[wave][k] = c4[k];
            }
            __syncthreads();
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const unsigned tot = (sh_cnt[0][k] + sh_cnt[1][k]) + (sh_cnt[2][k] + sh_cnt[3][k]);
                if (kk[k] >= tot) kk[k] -= tot, pre[k] |= 1ULL << bit;
            }
        }
        // a NaN among the values makes the percentile NaN, whatever the passes selected
        speed_p95 = nv ? nan : pct_lerp(unkey64(pre[0]), unkey64(pre[1]), gv);
        accel_p95 = na ? nan : pct_lerp(unkey64(pre[2]), unkey64(pre[3]), ga);
    }
    if (tid == 0) {
        double s = 0.0;
        int c = 0;
        for (int e = 0; e < E; ++e)
            if (sh_has[e]) {
                s += sh_cv[e];
                ++c;
            }
        // the mirror score of the last frame: pairs finite on both sides, in pair order
        double ms = 0.0;
        int mc = 0;
        if (n >= 1) {
            const double* fr = Xc + (long)(n - 1) * J * 3;
            for (int k = 0; k < a.P; ++k) {
                const double *l = fr + 3 * a.pairs[k][0], *r = fr + 3 * a.pairs[k][1];
                if (fin3(l) && fin3(r)) {
                    ms += norm3(l[0] - -r[0], l[1] - r[1], l[2] - r[2]);
                    ++mc;
                }
            }
        }
        out[SKIMI_CQ_BONE_CV_POOLED] = cv_pooled;
        out[SKIMI_CQ_BONE_CV_MEAN] = c > 0 ? s / (double)c : nan;
        out[SKIMI_CQ_LR_LENGTH_SYMMETRY] = lr_sym;
        out[SKIMI_CQ_SPEED_MEAN] = speed_mean;
        out[SKIMI_CQ_JERK_MEAN] = jerk_mean;
        out[SKIMI_CQ_SPEED_P95] = speed_p95;
        out[SKIMI_CQ_ACCEL_P95] = accel_p95;
        out[SKIMI_CQ_MIRROR_SYMMETRY] = mc > 0 ? ms / (double)mc : nan;
    }
}

inline bool eval_sizes_ok(int64_t clips, int64_t frames, int32_t joints) {
    return clips >= 0 && clips <= 0x7fffffffLL && frames >= 0 && frames <= 0x7fffffffLL - 64 && joints >= 1 && joints <= kMaxJoints &&
           clips * joints <= 0x7fffffffLL && (frames == 0 || (clips <= kMaxElems / frames / joints / 3 && clips * frames <= 0x7fffffffLL));
}

inline int copy_index_list(const int32_t* src, int32_t count, int32_t joints, uint8_t (*dst)[2], const char* what) {
    for (int k = 0; k < count; ++k)
        for (int s = 0; s < 2; ++s) {
            SKIMI_CHECK_ARG(src[2 * k + s] >= 0 && src[2 * k + s] < joints, "skimi_clip_quality: %s[%d][%d] = %d outside 0 .. joints - 1 = %d", what, k,
                            s, src[2 * k + s], joints - 1);
            dst[k][s] = (uint8_t)src[2 * k + s];
        }
    return SKIMI_OK;
}

}  // namespace
}  // namespace skimi

using namespace skimi;

extern "C" {

size_t skimi_eval_workspace_bytes(int64_t clips, int64_t frames, int32_t joints) {
    if (clips <= 0 || frames <= 0 || !eval_sizes_ok(clips, frames, joints)) return 0;
    return (size_t)clips * 5 * (size_t)frames * (size_t)joints * sizeof(double);
}

int skimi_pose_errors(const double* pred, const double* target, const int32_t* lengths, int64_t clips, int64_t frames, int32_t joints,
                      int32_t zero_root, double* err, double* p_err, double* vel_err, double* mpjpe_f, double* n_mpjpe_f,
                      double* p_mpjpe_f, int32_t* n_valid_f, int32_t* p_status, double* aligned, double* p_R, double* p_scale,
                      double* p_t, double* metrics, int32_t* counts, double* joint_stats, int32_t* joint_n, void* stream) {
    SKIMI_CHECK_ARG(eval_sizes_ok(clips, frames, joints),
                    "skimi_pose_errors: clips = %lld, frames = %lld, joints = %d outside 0 <= clips < 2^31, 0 <= frames < 2^31 - 64, 1 <= joints "
                    "<= %d, clips * frames < 2^31, clips * frames * joints * 3 <= 2^40", (long long)clips, (long long)frames, joints, kMaxJoints);
    SKIMI_CHECK_ARG(zero_root >= -1 && zero_root < joints, "skimi_pose_errors: zero_root = %d outside -1 .. joints - 1 = %d", zero_root,
                    joints - 1);
    if (clips == 0) return SKIMI_OK;
    SKIMI_CHECK_ARG(metrics && counts && joint_stats && joint_n, "skimi_pose_errors: NULL per-clip output");
    if (frames > 0)
        SKIMI_CHECK_ARG(pred && target && err && p_err && vel_err && mpjpe_f && n_mpjpe_f && p_mpjpe_f && n_valid_f && p_status,
                        "skimi_pose_errors: NULL input or per-frame output");
    PeArgs a;
    a.pred = pred, a.target = target, a.lengths = lengths;
    a.err = err, a.p_err = p_err, a.vel_err = vel_err, a.mpjpe_f = mpjpe_f, a.n_mpjpe_f = n_mpjpe_f, a.p_mpjpe_f = p_mpjpe_f;
    a.aligned = aligned, a.p_R = p_R, a.p_scale = p_scale, a.p_t = p_t, a.metrics = metrics, a.joint_stats = joint_stats;
    a.n_valid_f = n_valid_f, a.p_status = p_status, a.counts = counts, a.joint_n = joint_n;
    a.B = clips, a.T = frames, a.J = joints, a.zero_root = zero_root;
    hipStream_t st = (hipStream_t)stream;
    if (frames > 0) {
        hipLaunchKernelGGL(pe_frame_kernel, dim3((unsigned)cdiv(clips * frames, kWaves)), dim3(kThreads), 0, st, a);
        SKIMI_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(pe_clip_kernel, dim3((unsigned)clips), dim3(kThreads), 0, st, a);
    SKIMI_LAUNCH_CHECK();
    hipLaunchKernelGGL(pe_joint_kernel, dim3((unsigned)cdiv(clips * 2 * joints, kWaves)), dim3(kThreads), 0, st, a);
    SKIMI_LAUNCH_CHECK();
    return SKIMI_OK;
}

int skimi_clip_quality(const double* X, const int32_t* lengths, int64_t clips, int64_t frames, int32_t joints, const int32_t* edges,
                       int32_t n_edges, const int32_t* left_edges, int32_t n_left, const int32_t* right_edges, int32_t n_right,
                       const int32_t* lr_pairs, int32_t n_pairs, void* workspace, size_t workspace_bytes, double* scalars,
                       double* bone_cv_edge, double* bone_len, void* stream) {
    SKIMI_CHECK_ARG(eval_sizes_ok(clips, frames, joints),
                    "skimi_clip_quality: clips = %lld, frames = %lld, joints = %d outside 0 <= clips < 2^31, 0 <= frames < 2^31 - 64, 1 <= joints "
                    "<= %d, clips * frames < 2^31, clips * frames * joints * 3 <= 2^40", (long long)clips, (long long)frames, joints, kMaxJoints);
    SKIMI_CHECK_ARG(n_edges >= 0 && n_edges <= kMaxEdges && n_left >= 0 && n_left <= kMaxEdges && n_right >= 0 && n_right <= kMaxEdges &&
                        n_pairs >= 0 && n_pairs <= kMaxPairs,
                    "skimi_clip_quality: %d edges, %d left, %d right (at most %d each), %d pairs (at most %d)", n_edges, n_left, n_right,
                    kMaxEdges, n_pairs, kMaxPairs);
    SKIMI_CHECK_ARG((edges || !n_edges) && (left_edges || !n_left) && (right_edges || !n_right) && (lr_pairs || !n_pairs),
                    "skimi_clip_quality: NULL index list");
    CqArgs a;
    int rc;
    if ((rc = copy_index_list(edges, n_edges, joints, a.edges, "edges")) != SKIMI_OK) return rc;
    if ((rc = copy_index_list(left_edges, n_left, joints, a.ledges, "left_edges")) != SKIMI_OK) return rc;
    if ((rc = copy_index_list(right_edges, n_right, joints, a.redges, "right_edges")) != SKIMI_OK) return rc;
    if ((rc = copy_index_list(lr_pairs, n_pairs, joints, a.pairs, "lr_pairs")) != SKIMI_OK) return rc;
    if (clips == 0) return SKIMI_OK;
    SKIMI_CHECK_ARG(scalars && (bone_cv_edge || !n_edges), "skimi_clip_quality: NULL output");
    if (frames > 0) {
        SKIMI_CHECK_ARG(X, "skimi_clip_quality: NULL X");
        if (workspace)
            SKIMI_CHECK_ARG(workspace_bytes >= skimi_eval_workspace_bytes(clips, frames, joints) && ((uintptr_t)workspace & 7) == 0,
                            "skimi_clip_quality: the workspace has %zu bytes, skimi_eval_workspace_bytes asks for %zu (8-byte aligned)",
                            workspace_bytes, skimi_eval_workspace_bytes(clips, frames, joints));
        else
            SKIMI_CHECK_ARG(frames * joints <= SKIMI_EVAL_LDS_ELEMS, "skimi_clip_quality: frames * joints = %lld > %d needs a workspace",
                            (long long)(frames * joints), SKIMI_EVAL_LDS_ELEMS);
    }
    a.X = X, a.lengths = lengths;
    a.ws = frames > 0 ? (double*)workspace : nullptr;
    a.scalars = scalars, a.cv_edge = bone_cv_edge, a.bone_len = bone_len;
    a.B = clips, a.T = frames, a.stride = 5 * frames * joints;
    a.J = joints, a.E = n_edges, a.EL = n_left, a.ER = n_right, a.P = n_pairs;
    const size_t lds = a.ws ? 0 : (size_t)a.stride * sizeof(double);
    hipLaunchKernelGGL(clip_quality_kernel, dim3((unsigned)clips), dim3(kThreads), lds, (hipStream_t)stream, a);
    SKIMI_LAUNCH_CHECK();
    return SKIMI_OK;
}

}  // extern "C"
