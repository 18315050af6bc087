// Bird's-eye view of the front camera (DESIGN §2 "Bird's-eye view"): the homography of marked ground points onto a metric
// plane (cv2.findHomography(method=0) without its Levenberg-Marquardt polish), points through a homography, the
// perspective warp of uint8 frames (cv2.warpPerspective(INTER_LINEAR), constant border 0), the side views' skeleton placed
// on the plan and the metric ground track.  tests/bev_restated.py is the restatement: both sides evaluate every expression
// in the same order in float64 with no fused multiply-add (the build's -ffp-contract=off).
//
// One launch per call, no atomics, no host synchronisation, no allocation.  Every matrix a kernel reads (H, Hinv) lives in
// DEVICE memory, one per group / camera / frame: the fit, the inverse and the warp run back to back on a stream, and a
// panning camera has a matrix per frame.  Only `post` of the fit (the canvas matrix S of make_bev_canvas) comes from the
// host, by value.
#include "common.h"
#include "fp64_util.h"
#include "jacobi.h"
#include "reduce.h"   // wave_sum: the skeleton's centre
#include "warp_u8.h"

namespace skimi {

namespace {

constexpr int kFitThreads = 64;   // one wave per group
constexpr int kPtThreads = 256;
constexpr int kTrackThreads = 256;
constexpr int kSym = 45;   // the upper triangle of the 9 x 9 normal matrix

struct Mat3 {
    double m[9];
};

__device__ inline double det3(const double* H) {
    return H[0] * (H[4] * H[8] - H[5] * H[7]) - H[1] * (H[3] * H[8] - H[5] * H[6]) + H[2] * (H[3] * H[7] - H[4] * H[6]);
}

// (X, Y, w) = M (x, y, 1), each component as (m0 x + m1 y) + m2
__device__ __forceinline__ void apply3(const double* M, double x, double y, double& X, double& Y, double& w) {
    X = (M[0] * x + M[1] * y) + M[2];
    Y = (M[3] * x + M[4] * y) + M[5];
    w = (M[6] * x + M[7] * y) + M[8];
}

// ---- rule set 1: the fit, one wave per group -------------------------------------------------------------------------
// Every sum over the points is ONE lane's, in point order: lanes 0 .. 4 own the count and the four coordinate sums, lanes
// 0 .. 1 the two mean distances, lanes 0 .. 44 an entry each of the normal matrix's upper triangle (every lane re-reads the
// group's points, which the wave's first pass left in cache).  No tree, so nothing depends on n's relation to the wave
// and the restatement's point-order sums are the same bits.  The cost is a serial chain of n steps per sum, about a
// microsecond a point, on top of the 0.3 ms of the one-lane Jacobi (profiles/bev.md): ground points come by the handful
// and a fit is made once per clip, or once per frame with the frames' fits side by side in one launch.
__device__ __forceinline__ bool used4(const double* xs, const double* xd, int i) {
    return is_fin(xs[2 * i]) && is_fin(xs[2 * i + 1]) && is_fin(xd[2 * i]) && is_fin(xd[2 * i + 1]);
}

__global__ __launch_bounds__(kFitThreads) void homography_fit_kernel(const double* __restrict__ src, const double* __restrict__ dst,
                                                                     Mat3 post, int n, double* __restrict__ H_out, double* __restrict__ Hn_out,
                                                                     double* __restrict__ Hinv_out, double* __restrict__ err_out,
                                                                     double* __restrict__ stats_out, int* __restrict__ status_out) {
    __shared__ double sums[5], dist[2], M[81], Q[81], sH[9], s_err[kFitThreads];
    __shared__ int s_used[kFitThreads];
    __shared__ double s_det;
    __shared__ int s_ok;
    const int64_t g = blockIdx.x;
    const double* xs = src + g * n * 2;
    const double* xd = dst + g * n * 2;
    const int tid = threadIdx.x;

    // 1, 2: the used points, their centroids and mean distances
    if (tid < 5) {
        double acc = 0.0;
        for (int i = 0; i < n; ++i)
            if (used4(xs, xd, i)) acc += tid == 0 ? 1.0 : tid <= 2 ? xs[2 * i + tid - 1] : xd[2 * i + tid - 3];
        sums[tid] = acc;
    }
    __syncthreads();
    const double m = sums[0];
    const double cx = sums[1] / m, cy = sums[2] / m, cu = sums[3] / m, cv = sums[4] / m;
    if (tid < 2) {
        const double* pts = tid == 0 ? xs : xd;
        const double c0 = tid == 0 ? cx : cu, c1 = tid == 0 ? cy : cv;
        double acc = 0.0;
        for (int i = 0; i < n; ++i)
            if (used4(xs, xd, i)) {
                const double e0 = pts[2 * i] - c0, e1 = pts[2 * i + 1] - c1;
                acc += sqrt(e0 * e0 + e1 * e1);
            }
        dist[tid] = acc;
    }
    __syncthreads();
    const double ds = dist[0] / m, dd = dist[1] / m;
    const double ss = sqrt(2.0) / ds, sd = sqrt(2.0) / dd;
    const bool usable = m >= 4.0 && is_fin(ds) && is_fin(dd) && ds != 0.0 && dd != 0.0;   // wave-uniform

    // 3: entry (a, b), a <= b, of the normal matrix of the normalised system
    if (usable && tid < kSym) {
        int a = 0, k = tid;
        while (k >= 9 - a) k -= 9 - a, ++a;
        const int b = a + k;
        double acc = 0.0;
        for (int i = 0; i < n; ++i) {
            if (!used4(xs, xd, i)) continue;
            const double x = (xs[2 * i] - cx) * ss, y = (xs[2 * i + 1] - cy) * ss;
            const double u = (xd[2 * i] - cu) * sd, v = (xd[2 * i + 1] - cv) * sd;
            const double r1[9] = {-x, -y, -1.0, 0.0, 0.0, 0.0, u * x, u * y, u};
            const double r2[9] = {0.0, 0.0, 0.0, -x, -y, -1.0, v * x, v * y, v};
            double r1a = 0.0, r1b = 0.0, r2a = 0.0, r2b = 0.0;
#pragma unroll
            for (int e = 0; e < 9; ++e) {   // a register select, not an indexed array
                r1a = e == a ? r1[e] : r1a, r1b = e == b ? r1[e] : r1b;
                r2a = e == a ? r2[e] : r2a, r2b = e == b ? r2[e] : r2b;
            }
            acc += r1a * r1b + r2a * r2b;
        }
        M[a * 9 + b] = M[b * 9 + a] = acc;
    }
    __syncthreads();

    // 4 .. 8: one lane finishes the group
    if (tid == 0) {
        bool ok = usable;
        double Hn[9], det_n = qnan();
        if (ok) {
            jacobi_serial<9>(M, Q);
            int best = 0;
            for (int c = 1; c < 9; ++c)
                if (M[c * 9 + c] < M[best * 9 + best]) best = c;   // a tie keeps the lower index
            double h[9];
            for (int r = 0; r < 9; ++r) h[r] = Q[r * 9 + best];
            // 5: Hn = T_dst^-1 h T_src, T = [[s, 0, -s c_x], [0, s, -s c_y], [0, 0, 1]]
            double A[9];
            for (int r = 0; r < 3; ++r) {
                A[3 * r] = h[3 * r] * ss;
                A[3 * r + 1] = h[3 * r + 1] * ss;
                A[3 * r + 2] = (h[3 * r + 2] - A[3 * r] * cx) - A[3 * r + 1] * cy;
            }
            for (int c = 0; c < 3; ++c) {
                Hn[c] = A[c] / sd + cu * A[6 + c];
                Hn[3 + c] = A[3 + c] / sd + cv * A[6 + c];
                Hn[6 + c] = A[6 + c];
            }
            double fro = 0.0;
            for (int e = 0; e < 9; ++e) fro += Hn[e] * Hn[e];
            fro = sqrt(fro);
            if (fabs(Hn[8]) >= 1e-12 * fro) {
                const double h22 = Hn[8];
                for (int e = 0; e < 9; ++e) Hn[e] = Hn[e] / h22;
            } else {
                int big = 0;
                for (int e = 1; e < 9; ++e)
                    if (fabs(Hn[e]) > fabs(Hn[big])) big = e;
                const double sc = Hn[big] < 0.0 ? -fro : fro;
                for (int e = 0; e < 9; ++e) Hn[e] = Hn[e] / sc;
            }
            // 6: the reference's check_homography on H_m
            det_n = det3(Hn);
            bool fin = true;
            for (int e = 0; e < 9; ++e) fin = fin && is_fin(Hn[e]);
            ok = fin && is_fin(det_n) && fabs(det_n) >= 1e-12;
        }
        double Hi[9];
        if (ok) {
            // 7: H = post Hn, not renormalised;  8: Hinv = adj(H) / det(H)
            double Hc[9];
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 3; ++c)
                    Hc[3 * r + c] = (post.m[3 * r] * Hn[c] + post.m[3 * r + 1] * Hn[3 + c]) + post.m[3 * r + 2] * Hn[6 + c];
            const double det = det3(Hc);
            const double adj[9] = {Hc[4] * Hc[8] - Hc[5] * Hc[7], Hc[2] * Hc[7] - Hc[1] * Hc[8], Hc[1] * Hc[5] - Hc[2] * Hc[4],
                                   Hc[5] * Hc[6] - Hc[3] * Hc[8], Hc[0] * Hc[8] - Hc[2] * Hc[6], Hc[2] * Hc[3] - Hc[0] * Hc[5],
                                   Hc[3] * Hc[7] - Hc[4] * Hc[6], Hc[1] * Hc[6] - Hc[0] * Hc[7], Hc[0] * Hc[4] - Hc[1] * Hc[3]};
            for (int e = 0; e < 9; ++e) sH[e] = Hc[e], Hi[e] = adj[e] / det;
        } else {
            for (int e = 0; e < 9; ++e) sH[e] = Hi[e] = qnan();   // 9
        }
        s_ok = ok ? 1 : 0;
        s_det = det_n;
        for (int e = 0; e < 9; ++e) H_out[g * 9 + e] = sH[e], Hinv_out[g * 9 + e] = Hi[e];
        if (Hn_out)
            for (int e = 0; e < 9; ++e) Hn_out[g * 9 + e] = ok ? Hn[e] : qnan();
        status_out[g] = s_ok;
    }
    __syncthreads();

    // 10: the transfer error of every used point, against post x', a chunk of 64 points at a time: every lane computes its
    // point's error and leaves it in LDS, then lane 0 adds the chunk's squares in point order
    const bool ok = s_ok != 0;
    double e2 = 0.0, mx = 0.0;
    for (int base = 0; base < n; base += kFitThreads) {   // a wave-uniform trip count
        const int i = base + tid;
        double e = qnan();
        bool used = false;
        if (i < n) {
            used = ok && used4(xs, xd, i);
            if (used) {
                double X, Y, w, U, V, t;
                apply3(sH, xs[2 * i], xs[2 * i + 1], X, Y, w);
                apply3(post.m, xd[2 * i], xd[2 * i + 1], U, V, t);
                const double ex = X / w - U / t, ey = Y / w - V / t;
                e = sqrt(ex * ex + ey * ey);
            }
            err_out[g * n + i] = e;
        }
        s_err[tid] = e;
        s_used[tid] = used ? 1 : 0;
        __syncthreads();
        if (tid == 0)
            for (int k = 0; k < kFitThreads; ++k)
                if (s_used[k]) {
                    e2 += s_err[k] * s_err[k];
                    mx = max_nan(mx, s_err[k]);
                }
        __syncthreads();
    }
    if (tid == 0) {
        double* st = stats_out + g * 4;
        st[0] = m;
        st[1] = ok ? sqrt(e2 / m) : qnan();
        st[2] = ok ? mx : qnan();
        st[3] = s_det;
    }
}

// ---- rule set 2: points through a homography -------------------------------------------------------------------------
__global__ __launch_bounds__(kPtThreads) void homography_points_kernel(const double* __restrict__ x, const double* __restrict__ H,
                                                                       int64_t total_pts, int64_t n, int shared, double eps,
                                                                       double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kPtThreads + threadIdx.x;
    if (i >= total_pts) return;
    const double* h = shared ? H : H + (i / n) * 9;
    const double px = x[2 * i], py = x[2 * i + 1];
    double X, Y, w;
    apply3(h, px, py, X, Y, w);
    double ox = X / w, oy = Y / w;
    if (!(is_fin(px) && is_fin(py) && is_fin(w)) || fabs(w) < eps) ox = oy = qnan();
    out[2 * i] = ox;
    out[2 * i + 1] = oy;
}

// ---- rule set 3: the perspective warp --------------------------------------------------------------------------------
// lens.hip's undistort_u8_kernel with another source-position function: warp_u8.h holds what the two share.  The matrix
// of the image is nine doubles at a workgroup-uniform address, read once into registers (scalar loads).  X / w and Y / w
// are plain divisions, as cv2's: nothing tests the sign of w, so what lies beyond the horizon line is mirrored as cv2
// mirrors it.
template <int CH>
__global__ __launch_bounds__(kWarpX* kWarpY) void warp_perspective_u8_kernel(const unsigned char* __restrict__ in,
                                                                            unsigned char* __restrict__ out,
                                                                            const double* __restrict__ Hinv, int per_frame, int F,
                                                                            int H, int W, int OH, int OW, int aligned) {
    const int v = blockIdx.y * kWarpY + threadIdx.y;
    const int u0 = (blockIdx.x * kWarpX + threadIdx.x) * kPix;
    if (v >= OH || u0 >= OW) return;
    const int img = blockIdx.z;
    const double* gm = Hinv + (size_t)(per_frame ? img : img / F) * 9;
    double g[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) g[e] = gm[e];
    const unsigned char* src = in + (size_t)img * H * W * CH;
    const double vd = (double)v;
    unsigned int words[CH] = {};   // kPix * CH bytes, byte b of the span in word b / 4
#pragma unroll
    for (int p = 0; p < kPix; ++p) {
        const int u = u0 + p;
        double X, Y, w;
        apply3(g, (double)u, vd, X, Y, w);
        const double su = X / w, sv = Y / w;
        if (!(u < OW && warp_inside(su, sv, H, W))) continue;   // the bytes stay 0: the constant border; a NaN lands here
        warp_tap_pack<CH>(src, H, W, su, sv, p, words);
    }
    warp_store<CH>(out + (((size_t)img * OH + v) * OW + u0) * CH, words, aligned, u0, OW);
}

// ---- rule set 4: the skeleton on the plan, one wave per step -----------------------------------------------------------
__device__ inline int rint_i32(double x) {   // round half to even, saturating
    return (int)fmax(fmin(rint(x), 2147483647.0), -2147483648.0);
}

__global__ __launch_bounds__(64) void bev_skeleton_kernel(const double* __restrict__ X, const double* __restrict__ center_px,
                                                          const double* __restrict__ center_in, int J,
                                                          double mpp, int ax0, int ax1, int rot90_left, double* __restrict__ uv,
                                                          int* __restrict__ px, unsigned char* __restrict__ valid,
                                                          double* __restrict__ center_world) {
    const int64_t t = blockIdx.x;
    const int lane = threadIdx.x;
    const double* Xt = X + t * J * 3;
    // np.nanmean per coordinate: lane l adds its joints l, l + 64, .. in order, then the xor butterfly
    double s[3] = {0.0, 0.0, 0.0};
    int c[3] = {0, 0, 0};
    for (int j = lane; j < J; j += 64)
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double x = Xt[3 * j + a];
            if (x == x) s[a] += x, c[a] += 1;
        }
    double ctr[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double sum = wave_sum(s[a]);
        const int cnt = wave_sum(c[a]);
        ctr[a] = cnt > 0 ? sum / (double)cnt : qnan();
        if (center_in) ctr[a] = center_in[t * 3 + a];   // the caller's centre in place of the mean
    }
    if (lane < 3) center_world[t * 3 + lane] = lane == 0 ? ctr[0] : lane == 1 ? ctr[1] : ctr[2];
    const double cxw = ax0 == 0 ? ctr[0] : ax0 == 1 ? ctr[1] : ctr[2];
    const double czw = ax1 == 0 ? ctr[0] : ax1 == 1 ? ctr[1] : ctr[2];
    const double cu = center_px[2 * t], cv = center_px[2 * t + 1];
    const bool ctr_ok = is_fin(cxw) && is_fin(czw) && is_fin(cu) && is_fin(cv);
    const double u0 = rint(cu), v0 = rint(cv);
    for (int j = lane; j < J; j += 64) {
        const double* xj = Xt + 3 * j;
        const int64_t row = t * J + j;
        const bool ok = ctr_ok && is_fin(xj[0]) && is_fin(xj[1]) && is_fin(xj[2]);
        double fu = qnan(), fv = qnan();
        int iu = 0, iv = 0;
        if (ok) {
            double dx = xj[ax0] - cxw, dz = xj[ax1] - czw;
            if (rot90_left) {
                const double sw = dx;
                dx = dz, dz = sw;
            }
            const double du = dx / mpp, dv = -dz / mpp;
            fu = u0 + du, fv = v0 + dv;
            iu = rint_i32(fu), iv = rint_i32(fv);
        }
        uv[2 * row] = fu, uv[2 * row + 1] = fv;
        px[2 * row] = iu, px[2 * row + 1] = iv;
        valid[row] = ok ? 1 : 0;
    }
}

// ---- rule set 5: the ground track, one workgroup per person ------------------------------------------------------------
__device__ __forceinline__ bool fin2(const double* p) { return is_fin(p[0]) && is_fin(p[1]); }
__device__ __forceinline__ double step_of(const double* p, int64_t t) {
    if (t == 0) return 0.0;
    const double* a = p + 2 * (t - 1);
    const double* b = p + 2 * t;
    if (!(fin2(a) && fin2(b))) return qnan();
    const double dx = b[0] - a[0], dy = b[1] - a[1];
    return sqrt(dx * dx + dy * dy);
}

__global__ __launch_bounds__(kTrackThreads) void ground_track_kernel(const double* __restrict__ p_all, int64_t T, double fps,
                                                                     double* __restrict__ out_all) {
    const double* p = p_all + (int64_t)blockIdx.x * T * 2;
    double* out = out_all + (int64_t)blockIdx.x * T * 6;
    for (int64_t t = threadIdx.x; t < T; t += kTrackThreads) {
        double vx = qnan(), vy = qnan();
        if (T > 1) {
            const int64_t lo = t == 0 ? 0 : t - 1, hi = t == T - 1 ? t : t + 1;
            const double* a = p + 2 * lo;
            const double* b = p + 2 * hi;
            if (fin2(a) && fin2(b)) {
                vx = (b[0] - a[0]) * fps, vy = (b[1] - a[1]) * fps;
                if (hi - lo == 2) vx = vx / 2.0, vy = vy / 2.0;
            }
        }
        double* o = out + 6 * t;
        o[0] = step_of(p, t);
        o[2] = vx, o[3] = vy;
        o[4] = sqrt(vx * vx + vy * vy);
        o[5] = atan2(vx, vy);
    }
    if (threadIdx.x == 0) {   // the running sum of the finite steps, in time order
        double path = 0.0;
        for (int64_t t = 0; t < T; ++t) {
            const double s = step_of(p, t);
            if (is_fin(s)) path += s;
            out[6 * t + 1] = path;
        }
    }
}

int check_frames(const char* what, int32_t C, int32_t F, int32_t H, int32_t W, int32_t OH, int32_t OW, int32_t ch) {
    SKIMI_CHECK_ARG(ch == 1 || ch == 3 || ch == 4, "%s: %d channels (1, 3 or 4)", what, ch);
    SKIMI_CHECK_ARG(C >= 1 && F >= 0 && (int64_t)C * F <= 65535, "%s: C = %d, C * F = %lld outside C >= 1, 0 .. 65535", what, C,
                    (long long)C * F);
    SKIMI_CHECK_ARG(H >= 1 && W >= 1 && OH >= 1 && OW >= 1 && H <= SKIMI_LENS_MAX_SIDE && W <= SKIMI_LENS_MAX_SIDE &&
                        OH <= SKIMI_LENS_MAX_SIDE && OW <= SKIMI_LENS_MAX_SIDE,
                    "%s: frame %d x %d -> %d x %d outside 1 .. %d a side", what, W, H, OW, OH, SKIMI_LENS_MAX_SIDE);
    return SKIMI_OK;
}

}  // namespace

}  // namespace skimi

using namespace skimi;

extern "C" {

int skimi_homography_fit(const double* src, const double* dst, const double* post, int64_t G, int32_t n, double* H, double* Hinv,
                         double* Hn, double* err, double* stats, int32_t* status, void* stream) {
    SKIMI_CHECK_ARG(G >= 1 && G <= 2147483647LL, "skimi_homography_fit: G = %lld outside 1 .. 2^31 - 1", (long long)G);
    SKIMI_CHECK_ARG(n >= 4 && G <= ((int64_t)1 << 31) / n, "skimi_homography_fit: n = %d, G = %lld outside 4 <= n, G * n <= 2^31", n,
                    (long long)G);
    SKIMI_CHECK_ARG(src && dst && H && Hinv && err && stats && status, "skimi_homography_fit: NULL points or outputs");
    Mat3 pm = {{1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}};
    if (post)
        for (int e = 0; e < 9; ++e) {
            SKIMI_CHECK_ARG(is_fin(post[e]), "skimi_homography_fit: post[%d] is not finite", e);
            pm.m[e] = post[e];
        }
    hipLaunchKernelGGL(homography_fit_kernel, dim3((unsigned)G), dim3(kFitThreads), 0, (hipStream_t)stream, src, dst, pm, n, H, Hn, Hinv,
                       err, stats, status);
    SKIMI_LAUNCH_CHECK();
    return SKIMI_OK;
}

int skimi_homography_points(const double* x, const double* H, int64_t G, int64_t n, int32_t shared, double eps, double* out,
                            void* stream) {
    SKIMI_CHECK_ARG(G >= 0 && n >= 0 && (n == 0 || G <= ((int64_t)1 << 31) / n),
                    "skimi_homography_points: G = %lld, n = %lld outside 0 <= G * n <= 2^31", (long long)G, (long long)n);
    SKIMI_CHECK_ARG(eps >= 0.0, "skimi_homography_points: eps must be a number >= 0");
    if (G * n == 0) return SKIMI_OK;
    SKIMI_CHECK_ARG(x && H && out, "skimi_homography_points: NULL points, matrices or output");
    hipLaunchKernelGGL(homography_points_kernel, dim3((unsigned)cdiv(G * n, kPtThreads)), dim3(kPtThreads), 0, (hipStream_t)stream,
                       x, H, G * n, n, shared, eps, out);
    SKIMI_LAUNCH_CHECK();
    return SKIMI_OK;
}

int skimi_warp_perspective_u8(const uint8_t* in, uint8_t* out, const double* Hinv, int32_t per_frame, int32_t C, int32_t F, int32_t H,
                              int32_t W, int32_t OH, int32_t OW, int32_t ch, void* stream) {
    const int rc = check_frames("skimi_warp_perspective_u8", C, F, H, W, OH, OW, ch);
    if (rc != SKIMI_OK) return rc;
    if (F == 0) return SKIMI_OK;
    SKIMI_CHECK_ARG(in && out && Hinv, "skimi_warp_perspective_u8: NULL frames or matrices");
    const int aligned = ((int64_t)OW * ch) % 4 == 0 && ((uintptr_t)out & 3) == 0;
    const int pf = per_frame != 0;
    const dim3 grid((unsigned)cdiv(OW, kWarpX * kPix), (unsigned)cdiv(OH, kWarpY), (unsigned)(C * F)), block(kWarpX, kWarpY);
    if (ch == 1)
        hipLaunchKernelGGL(warp_perspective_u8_kernel<1>, grid, block, 0, (hipStream_t)stream, in, out, Hinv, pf, F, H, W, OH, OW,
                           aligned);
    else if (ch == 3)
        hipLaunchKernelGGL(warp_perspective_u8_kernel<3>, grid, block, 0, (hipStream_t)stream, in, out, Hinv, pf, F, H, W, OH, OW,
                           aligned);
    else
        hipLaunchKernelGGL(warp_perspective_u8_kernel<4>, grid, block, 0, (hipStream_t)stream, in, out, Hinv, pf, F, H, W, OH, OW,
                           aligned);
    SKIMI_LAUNCH_CHECK();
    return SKIMI_OK;
}

int skimi_bev_skeleton(const double* X, const double* center_px, const double* center_world_in, int64_t T, int32_t J,
                       double metres_per_pixel, int32_t ax0, int32_t ax1, int32_t rot90_left, double* uv, int32_t* px, uint8_t* valid,
                       double* center_world, void* stream) {
    SKIMI_CHECK_ARG(T >= 0 && T <= 2147483647LL && J >= 1 && T <= ((int64_t)1 << 31) / J,
                    "skimi_bev_skeleton: T = %lld, J = %d outside 0 <= T, 1 <= J, T * J <= 2^31", (long long)T, J);
    SKIMI_CHECK_ARG(ax0 >= 0 && ax0 <= 2 && ax1 >= 0 && ax1 <= 2, "skimi_bev_skeleton: axes (%d, %d) outside 0 .. 2", ax0, ax1);
    SKIMI_CHECK_ARG(is_fin(metres_per_pixel) && metres_per_pixel > 0.0, "skimi_bev_skeleton: metres_per_pixel must be positive");
    if (T == 0) return SKIMI_OK;
    SKIMI_CHECK_ARG(X && center_px && uv && px && valid && center_world, "skimi_bev_skeleton: NULL inputs or outputs");
    hipLaunchKernelGGL(bev_skeleton_kernel, dim3((unsigned)T), dim3(64), 0, (hipStream_t)stream, X, center_px, center_world_in, J,
                       metres_per_pixel,
                       ax0, ax1, rot90_left != 0, uv, px, valid, center_world);
    SKIMI_LAUNCH_CHECK();
    return SKIMI_OK;
}

int skimi_ground_track(const double* p, int64_t P, int64_t T, double fps, double* out, void* stream) {
    SKIMI_CHECK_ARG(P >= 0 && P <= 2147483647LL && T >= 0 && (T == 0 || P <= ((int64_t)1 << 31) / T),
                    "skimi_ground_track: P = %lld, T = %lld outside 0 <= P * T <= 2^31", (long long)P, (long long)T);
    SKIMI_CHECK_ARG(is_fin(fps) && fps > 0.0, "skimi_ground_track: fps must be positive");
    if (P * T == 0) return SKIMI_OK;
    SKIMI_CHECK_ARG(p && out, "skimi_ground_track: NULL track or output");
    hipLaunchKernelGGL(ground_track_kernel, dim3((unsigned)P), dim3(kTrackThreads), 0, (hipStream_t)stream, p, T, fps, out);
    SKIMI_LAUNCH_CHECK();
    return SKIMI_OK;
}

}  // extern "C"
