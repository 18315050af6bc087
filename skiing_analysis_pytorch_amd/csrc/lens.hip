// Lens distortion (DESIGN §2 "Lens distortion"): OpenCV's rational + tangential + thin-prism model on keypoints and on
// whole frames.  skimi_distort_points / skimi_undistort_points / skimi_project_points move points between the ideal
// pinhole and the real lens, skimi_undistort_u8 warps uint8 frames with the source position of every output pixel
// computed on the fly.  tests/lens_restated.py is the restatement: both sides evaluate every expression in the same
// order in float64 with no fused multiply-add (the build's -ffp-contract=off), so they agree to the last bit.
//
// One launch per call.  The per-camera parameters (fx, fy, cx, cy of K and of the second matrix, twelve coefficients,
// R and t for the projection) travel BY VALUE in the kernel arguments, at most SKIMI_LENS_MAX_CAMERAS cameras a call:
// the kernels read them through the scalar unit with a workgroup-uniform index and load no table from memory.  The one
// exception is K_steps of the point calls, a device table of per-(step, camera) intrinsics for keypoints whose K is a
// model output that never left the device (geometry.triangulate_triage(dist=)).
#include "common.h"
#include "fp64_util.h"
#include "warp_u8.h"

namespace skimi {

namespace {

constexpr int kPtThreads = 256;

struct LensCam {
    double fx, fy, cx, cy;      // K
    double qfx, qfy, qcx, qcy;  // the second matrix: P of the point calls, new_K of the frame warp
    double d[12];               // k1 k2 p1 p2 k3 k4 k5 k6 s1 s2 s3 s4
};
struct LensCams {
    LensCam c[SKIMI_LENS_MAX_CAMERAS];
};
struct LensPose {
    double R[9], t[3];
};
struct LensPoses {
    LensPose c[SKIMI_LENS_MAX_CAMERAS];
};

// numerator and denominator of the radial factor c
__device__ inline void radial(const double* d, double r2, double r4, double& num, double& den) {
    const double r6 = r4 * r2;
    num = 1.0 + d[0] * r2 + d[1] * r4 + d[4] * r6;
    den = 1.0 + d[5] * r2 + d[6] * r4 + d[7] * r6;
}
// tangential + thin-prism terms
__device__ inline void tangential(const double* d, double x, double y, double r2, double r4, double& dx, double& dy) {
    const double a = (2.0 * x) * y;
    dx = d[2] * a + d[3] * (r2 + (2.0 * x) * x) + d[8] * r2 + d[9] * r4;
    dy = d[2] * (r2 + (2.0 * y) * y) + d[3] * a + d[10] * r2 + d[11] * r4;
}
__device__ inline void distort(const double* d, double x, double y, double& xd, double& yd) {
    const double r2 = x * x + y * y, r4 = r2 * r2;
    double num, den, dx, dy;
    radial(d, r2, r4, num, den);
    tangential(d, x, y, r2, r4, dx, dy);
    const double c = num / den;
    xd = x * c + dx;
    yd = y * c + dy;
}

// the camera of a point: its by-value record, K (and P = K) replaced by row (o, cam) of K_steps when that is given
__device__ inline void point_camera(const LensCams& cams, const double* K_steps, int64_t o, int C, int cam, double* k, double* q,
                                    double* d) {
    const LensCam& lc = cams.c[cam];
    k[0] = lc.fx, k[1] = lc.fy, k[2] = lc.cx, k[3] = lc.cy;
    q[0] = lc.qfx, q[1] = lc.qfy, q[2] = lc.qcx, q[3] = lc.qcy;
#pragma unroll
    for (int i = 0; i < 12; ++i) d[i] = lc.d[i];
    if (K_steps) {
        const double* Ks = K_steps + (o * C + cam) * 9;
        k[0] = q[0] = Ks[0], k[1] = q[1] = Ks[4], k[2] = q[2] = Ks[2], k[3] = q[3] = Ks[5];
    }
}

// points [outer, C, n, 2]: blockIdx.y = camera, the threads of a row of blocks walk the outer * n points of that camera
__global__ __launch_bounds__(kPtThreads) void distort_points_kernel(const double* __restrict__ in, double* __restrict__ out,
                                                                    LensCams cams, const double* __restrict__ K_steps,
                                                                    int64_t outer, int C, int64_t n, int normalized) {
    const int cam = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * kPtThreads + threadIdx.x;
    if (i >= outer * n) return;
    const int64_t o = i / n, j = i - o * n, p = ((o * C + cam) * n + j) * 2;
    double k[4], q[4], d[12];
    point_camera(cams, K_steps, o, C, cam, k, q, d);
    double x = in[p], y = in[p + 1];
    if (!normalized) {
        x = (x - q[2]) / q[0];
        y = (y - q[3]) / q[1];
    }
    double xd, yd;
    distort(d, x, y, xd, yd);
    out[p] = k[0] * xd + k[2];
    out[p + 1] = k[1] * yd + k[3];
}

__global__ __launch_bounds__(kPtThreads) void undistort_points_kernel(const double* __restrict__ in, double* __restrict__ out,
                                                                      double* __restrict__ resid, LensCams cams,
                                                                      const double* __restrict__ K_steps, int64_t outer, int C,
                                                                      int64_t n, int iters, int normalized) {
    const int cam = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * kPtThreads + threadIdx.x;
    if (i >= outer * n) return;
    const int64_t o = i / n, j = i - o * n, row = (o * C + cam) * n + j;
    double k[4], q[4], d[12];
    point_camera(cams, K_steps, o, C, cam, k, q, d);
    const double xd = (in[2 * row] - k[2]) / k[0], yd = (in[2 * row + 1] - k[3]) / k[1];
    double x = xd, y = yd;
    for (int it = 0; it < iters; ++it) {   // a fixed count, no data-dependent exit
        const double r2 = x * x + y * y, r4 = r2 * r2;
        double num, den, dx, dy;
        radial(d, r2, r4, num, den);
        tangential(d, x, y, r2, r4, dx, dy);
        const double ic = den / num;
        x = (xd - dx) * ic;
        y = (yd - dy) * ic;
    }
    double xr, yr;
    distort(d, x, y, xr, yr);
    const double du = k[0] * (xr - xd), dv = k[1] * (yr - yd);
    double r = sqrt(du * du + dv * dv);
    double ox = x, oy = y;
    if (!normalized) {
        ox = q[0] * x + q[2];
        oy = q[1] * y + q[3];
    }
    if (!(is_fin(ox) && is_fin(oy) && is_fin(r))) ox = oy = r = qnan();
    out[2 * row] = ox;
    out[2 * row + 1] = oy;
    resid[row] = r;
}

// X [outer, C, n, 3] -> px [outer, C, n, 2], depth [outer, C, n]
__global__ __launch_bounds__(kPtThreads) void project_points_kernel(const double* __restrict__ X, double* __restrict__ px,
                                                                    double* __restrict__ depth, LensCams cams, LensPoses poses,
                                                                    int64_t outer, int C, int64_t n) {
    const int cam = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * kPtThreads + threadIdx.x;
    if (i >= outer * n) return;
    const int64_t o = i / n, j = i - o * n, row = (o * C + cam) * n + j;
    const LensCam& lc = cams.c[cam];
    const LensPose& ps = poses.c[cam];
    double d[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) d[e] = lc.d[e];
    const double X0 = X[3 * row], X1 = X[3 * row + 1], X2 = X[3 * row + 2];
    const double xc = ps.R[0] * X0 + ps.R[1] * X1 + ps.R[2] * X2 + ps.t[0];
    const double yc = ps.R[3] * X0 + ps.R[4] * X1 + ps.R[5] * X2 + ps.t[1];
    const double zc = ps.R[6] * X0 + ps.R[7] * X1 + ps.R[8] * X2 + ps.t[2];
    double xd, yd;
    distort(d, xc / zc, yc / zc, xd, yd);
    px[2 * row] = lc.fx * xd + lc.cx;
    px[2 * row + 1] = lc.fy * yd + lc.cy;
    depth[row] = zc;
}

// ---- the frame warp ------------------------------------------------------------------------------------------------
// in [C, F, H, W, CH] -> out [C, F, OH, OW, CH].  The thread shape, the taps, the rounding and the stores are warp_u8.h's
// (shared with bev.hip's perspective warp); this kernel supplies the source position.  A wave covers 64 * kPix = 256
// adjacent pixels of a row, so its gathers fall into the two source rows around the (gently curved) preimage of that
// span: a few cache lines a row.  blockIdx.z = (camera, frame).
template <int CH>
__global__ __launch_bounds__(kWarpX* kWarpY) void undistort_u8_kernel(const unsigned char* __restrict__ in,
                                                                     unsigned char* __restrict__ out, LensCams cams, int F, int H,
                                                                     int W, int OH, int OW, int aligned) {
    const int v = blockIdx.y * kWarpY + threadIdx.y;
    const int u0 = (blockIdx.x * kWarpX + threadIdx.x) * kPix;
    if (v >= OH || u0 >= OW) return;
    const int img = blockIdx.z, cam = img / F;
    const LensCam& lc = cams.c[cam];
    double d[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) d[e] = lc.d[e];
    const unsigned char* src = in + (size_t)img * H * W * CH;
    const double y = ((double)v - lc.qcy) / lc.qfy;
    unsigned int words[CH] = {};   // kPix * CH bytes, byte b of the span in word b / 4
#pragma unroll
    for (int p = 0; p < kPix; ++p) {
        const int u = u0 + p;
        const double x = ((double)u - lc.qcx) / lc.qfx;
        double xd, yd;
        distort(d, x, y, xd, yd);
        const double su = lc.fx * xd + lc.cx, sv = lc.fy * yd + lc.cy;
        if (!(u < OW && warp_inside(su, sv, H, W))) continue;   // the bytes stay 0: the constant border
        warp_tap_pack<CH>(src, H, W, su, sv, p, words);
    }
    warp_store<CH>(out + (((size_t)img * OH + v) * OW + u0) * CH, words, aligned, u0, OW);
}

// host side: K [C, 3, 3], the second matrix (NULL: K), dist [C, 12] -> the by-value records
int pack_cams(const char* what, int32_t C, const double* K, const double* Q, const double* dist, bool need_K, LensCams& cams) {
    SKIMI_CHECK_ARG(C >= 1 && C <= SKIMI_LENS_MAX_CAMERAS, "%s: %d cameras outside 1 .. %d", what, C, SKIMI_LENS_MAX_CAMERAS);
    SKIMI_CHECK_ARG(K || !need_K, "%s: NULL K", what);
    for (int c = 0; c < C; ++c) {
        LensCam& lc = cams.c[c];
        const double* k = K ? K + 9 * c : nullptr;
        const double* q = Q ? Q + 9 * c : k;
        lc.fx = k ? k[0] : 1.0, lc.fy = k ? k[4] : 1.0, lc.cx = k ? k[2] : 0.0, lc.cy = k ? k[5] : 0.0;
        lc.qfx = q ? q[0] : 1.0, lc.qfy = q ? q[4] : 1.0, lc.qcx = q ? q[2] : 0.0, lc.qcy = q ? q[5] : 0.0;
        SKIMI_CHECK_ARG(is_fin(lc.fx) && is_fin(lc.fy) && is_fin(lc.cx) && is_fin(lc.cy) && lc.fx != 0.0 && lc.fy != 0.0 &&
                            is_fin(lc.qfx) && is_fin(lc.qfy) && is_fin(lc.qcx) && is_fin(lc.qcy) && lc.qfx != 0.0 && lc.qfy != 0.0,
                        "%s: camera %d has a zero or non-finite focal length or principal point", what, c);
        for (int e = 0; e < 12; ++e) {
            lc.d[e] = dist ? dist[12 * c + e] : 0.0;
            SKIMI_CHECK_ARG(is_fin(lc.d[e]), "%s: coefficient %d of camera %d is not finite", what, e, c);
        }
    }
    return SKIMI_OK;
}

int check_points(const char* what, int64_t outer, int64_t n) {
    SKIMI_CHECK_ARG(outer >= 0 && n >= 0 && (n == 0 || outer <= ((int64_t)1 << 31) / n),
                    "%s: outer = %lld, n = %lld outside 0 <= outer * n <= 2^31", what, (long long)outer, (long long)n);
    return SKIMI_OK;
}

}  // namespace

}  // namespace skimi

using namespace skimi;

extern "C" {

int skimi_distort_points(const double* x, const double* K, const double* dist, const double* P, const double* K_steps,
                         int64_t outer, int32_t C, int64_t n, int32_t normalized, double* out, void* stream) {
    LensCams cams;
    int rc = pack_cams("skimi_distort_points", C, K, P, dist, !K_steps, cams);
    if (rc != SKIMI_OK) return rc;
    if ((rc = check_points("skimi_distort_points", outer, n)) != SKIMI_OK) return rc;
    SKIMI_CHECK_ARG(!(K_steps && P), "skimi_distort_points: K_steps sets P = K, P must be NULL");
    if (outer * n == 0) return SKIMI_OK;
    SKIMI_CHECK_ARG(x && out, "skimi_distort_points: NULL points");
    hipLaunchKernelGGL(distort_points_kernel, dim3((unsigned)cdiv(outer * n, kPtThreads), (unsigned)C), dim3(kPtThreads), 0,
                       (hipStream_t)stream, x, out, cams, K_steps, outer, C, n, normalized);
    SKIMI_LAUNCH_CHECK();
    return SKIMI_OK;
}

int skimi_undistort_points(const double* x, const double* K, const double* dist, const double* P, const double* K_steps,
                           int64_t outer, int32_t C, int64_t n, int32_t iters, int32_t normalized, double* out, double* resid_px,
                           void* stream) {
    LensCams cams;
    int rc = pack_cams("skimi_undistort_points", C, K, P, dist, !K_steps, cams);
    if (rc != SKIMI_OK) return rc;
    if ((rc = check_points("skimi_undistort_points", outer, n)) != SKIMI_OK) return rc;
    SKIMI_CHECK_ARG(!(K_steps && P), "skimi_undistort_points: K_steps sets P = K, P must be NULL");
    SKIMI_CHECK_ARG(iters >= 0 && iters <= SKIMI_LENS_MAX_ITERS, "skimi_undistort_points: iters = %d outside 0 .. %d", iters,
                    SKIMI_LENS_MAX_ITERS);
    if (outer * n == 0) return SKIMI_OK;
    SKIMI_CHECK_ARG(x && out && resid_px, "skimi_undistort_points: NULL points or outputs");
    hipLaunchKernelGGL(undistort_points_kernel, dim3((unsigned)cdiv(outer * n, kPtThreads), (unsigned)C), dim3(kPtThreads), 0,
                       (hipStream_t)stream, x, out, resid_px, cams, K_steps, outer, C, n, iters, normalized);
    SKIMI_LAUNCH_CHECK();
    return SKIMI_OK;
}

int skimi_project_points(const double* X, const double* R, const double* t, const double* K, const double* dist, int64_t outer,
                         int32_t C, int64_t n, double* px, double* depth, void* stream) {
    LensCams cams;
    int rc = pack_cams("skimi_project_points", C, K, nullptr, dist, true, cams);
    if (rc != SKIMI_OK) return rc;
    if ((rc = check_points("skimi_project_points", outer, n)) != SKIMI_OK) return rc;
    SKIMI_CHECK_ARG(R && t, "skimi_project_points: NULL R or t");
    LensPoses poses;
    for (int c = 0; c < C; ++c) {
        for (int e = 0; e < 9; ++e) poses.c[c].R[e] = R[9 * c + e];
        for (int e = 0; e < 3; ++e) poses.c[c].t[e] = t[3 * c + e];
    }
    if (outer * n == 0) return SKIMI_OK;
    SKIMI_CHECK_ARG(X && px && depth, "skimi_project_points: NULL points or outputs");
    hipLaunchKernelGGL(project_points_kernel, dim3((unsigned)cdiv(outer * n, kPtThreads), (unsigned)C), dim3(kPtThreads), 0,
                       (hipStream_t)stream, X, px, depth, cams, poses, outer, C, n);
    SKIMI_LAUNCH_CHECK();
    return SKIMI_OK;
}

int skimi_undistort_u8(const uint8_t* in, uint8_t* out, const double* K, const double* dist, const double* new_K, int32_t C,
                       int32_t F, int32_t H, int32_t W, int32_t OH, int32_t OW, int32_t ch, void* stream) {
    LensCams cams;
    const int rc = pack_cams("skimi_undistort_u8", C, K, new_K, dist, true, cams);
    if (rc != SKIMI_OK) return rc;
    SKIMI_CHECK_ARG(ch == 1 || ch == 3 || ch == 4, "skimi_undistort_u8: %d channels (1, 3 or 4)", ch);
    SKIMI_CHECK_ARG(F >= 0 && (int64_t)C * F <= 65535, "skimi_undistort_u8: C * F = %lld outside 0 .. 65535", (long long)C * F);
    SKIMI_CHECK_ARG(H >= 1 && W >= 1 && OH >= 1 && OW >= 1 && H <= SKIMI_LENS_MAX_SIDE && W <= SKIMI_LENS_MAX_SIDE &&
                        OH <= SKIMI_LENS_MAX_SIDE && OW <= SKIMI_LENS_MAX_SIDE,
                    "skimi_undistort_u8: frame %d x %d -> %d x %d outside 1 .. %d a side", W, H, OW, OH, SKIMI_LENS_MAX_SIDE);
    if (F == 0) return SKIMI_OK;
    SKIMI_CHECK_ARG(in && out, "skimi_undistort_u8: NULL frames");
    const int aligned = ((int64_t)OW * ch) % 4 == 0 && ((uintptr_t)out & 3) == 0;
    const dim3 grid((unsigned)cdiv(OW, kWarpX * kPix), (unsigned)cdiv(OH, kWarpY), (unsigned)(C * F)), block(kWarpX, kWarpY);
    if (ch == 1)
        hipLaunchKernelGGL(undistort_u8_kernel<1>, grid, block, 0, (hipStream_t)stream, in, out, cams, F, H, W, OH, OW, aligned);
    else if (ch == 3)
        hipLaunchKernelGGL(undistort_u8_kernel<3>, grid, block, 0, (hipStream_t)stream, in, out, cams, F, H, W, OH, OW, aligned);
    else
        hipLaunchKernelGGL(undistort_u8_kernel<4>, grid, block, 0, (hipStream_t)stream, in, out, cams, F, H, W, OH, OW, aligned);
    SKIMI_LAUNCH_CHECK();
    return SKIMI_OK;
}

}  // extern "C"
