// Chessboard corner detection on whole frames (camera_calibration/main.py:80-90, find_chessboard_corners =
// cv2.findChessboardCorners + cv2.cornerSubPix) under the project's own rules: DESIGN §2 "Chessboard corners", the block in
// include/skimi.h; tests/chessboard_restated.py evaluates the same expressions.
//   response    one launch: gray (cv2's 8-bit BGR weights), 3 x 3 binomial blur, the ChESS response on the radius-5 ring
//               (Bennett & Lasenby) in int32, the frame's maximum by an integer atomic
//   candidates  compact.h's count / write launches: threshold against the frame's maximum, non-maximum suppression
//               with a raster-order tie rule, compaction in pixel order
//   subpix      cv2.cornerSubPix's iteration in float64, a fixed number of rounds, one wave a point, the patch in LDS
// Integer stages are exact and order-independent; the refinement's sums are reduce.h's wave_sum over a fixed lane
// assignment: every result is bitwise reproducible and a frame's results do not depend on the batch around it.
#include <math.h>

#include "common.h"
#include "compact.h"
#include "fp64_util.h"
#include "reduce.h"

namespace skimi {

constexpr int kChessThreads = 256;
constexpr int kChessTW = 64, kChessTH = 32;   // response pixels of a workgroup
constexpr int kChessHalo = 6;                 // ring radius 5 + blur radius 1
constexpr int kChessGW = kChessTW + 2 * kChessHalo, kChessGH = kChessTH + 2 * kChessHalo;   // gray tile 76 x 44
constexpr int kChessBW = kChessGW - 2, kChessBH = kChessGH - 2;                             // blur tile 74 x 42
constexpr int kChessRawDw = kChessGW + 2;     // dwords of a raw row: 76 px x 4 bytes + the misaligned ends
constexpr int kChessGS = 80;                  // bytes of a gray row in LDS: the blur reads it as dwords, four pixels a thread
constexpr int kChessBS = 76;                  // 16-bit values of a blur row in LDS: four of them are one 8-byte store
constexpr long kChessTile = 4096;             // pixels of a workgroup of the candidate launches
constexpr int kChessWaves = kChessThreads / 64;
constexpr int kSubpixPatch = 2 * SKIMI_SUBPIX_MAX_WIN + 3, kSubpixFoot = kSubpixPatch + 1;

template <int CH>
__device__ __forceinline__ int chess_gray(const unsigned char* p) {
    if (CH == 1) return p[0];
    return (3735 * (int)p[0] + 19235 * (int)p[1] + 9798 * (int)p[2] + 16384) >> 15;
}
__device__ __forceinline__ int chess_gray(const unsigned char* p, int ch) { return ch == 1 ? chess_gray<1>(p) : chess_gray<3>(p); }

__device__ __forceinline__ int wave_max_i32(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    return v;
}

// ---- launch 1: gray, blur, response, frame maximum ----
// grid (ceil(W / 64), ceil(H / 32), frames).  The rows of the gray tile's footprint are fetched as aligned dwords (the
// dword that holds a row's first or last byte lies in the page of that byte), converted to gray in LDS, blurred in LDS.
template <int CH>
__global__ __launch_bounds__(kChessThreads) void chess_response_kernel(const unsigned char* __restrict__ frames, int H, int W,
                                                                       int* __restrict__ resp, int* __restrict__ rmax) {
    // the raw rows are dead once they are gray: the blur tile takes their place
    __shared__ __attribute__((aligned(8))) unsigned s_raw[kChessGH][kChessRawDw];
    __shared__ __attribute__((aligned(8))) unsigned char s_gray[kChessGH][kChessGS];
    static_assert(sizeof(unsigned short) * kChessBH * kChessBS <= sizeof(unsigned) * kChessGH * kChessRawDw, "blur tile over the raw rows");
    unsigned short(*s_blur)[kChessBS] = reinterpret_cast<unsigned short(*)[kChessBS]>(&s_raw[0][0]);
    const int tid = threadIdx.x;
    const long f = blockIdx.z;
    const int x0 = (int)blockIdx.x * kChessTW - kChessHalo, y0 = (int)blockIdx.y * kChessTH - kChessHalo;
    const unsigned char* fp = frames + f * H * W * CH;
    const int xa = max(x0, 0), xb = min(x0 + kChessGW, W);   // the columns of the footprint inside the frame: xa < xb
    for (int idx = tid; idx < kChessGH * kChessRawDw; idx += kChessThreads) {
        const int r = idx / kChessRawDw, i = idx - r * kChessRawDw, gy = y0 + r;
        if (gy < 0 || gy >= H) continue;
        const uintptr_t p = (uintptr_t)(fp + ((long)gy * W + xa) * CH), a0 = p & ~(uintptr_t)3;
        const int ndw = (int)((p + (uintptr_t)(xb - xa) * CH + 3 - a0) >> 2);   // <= 76 + 1
        if (i < ndw) s_raw[r][i] = reinterpret_cast<const unsigned*>(a0)[i];
    }
    __syncthreads();
    const unsigned fp_low = (unsigned)(uintptr_t)fp;
    for (int idx = tid; idx < kChessGH * kChessGS; idx += kChessThreads) {
        const int r = idx / kChessGS, c = idx - r * kChessGS, gx = x0 + c, gy = y0 + r;
        int g = 0;   // outside the frame and in the row's padding
        if (c < kChessGW && gx >= 0 && gx < W && gy >= 0 && gy < H) {
            const int skew = (int)((fp_low + (unsigned)((gy * W + xa) * CH)) & 3u);   // the row's first byte in its first dword
            g = chess_gray<CH>(reinterpret_cast<const unsigned char*>(s_raw[r]) + skew + (gx - xa) * CH);
        }
        s_gray[r][c] = (unsigned char)g;
    }
    __syncthreads();
    // four blur values a thread from two dwords of each of three gray rows; the last group's two spare values are never read
    for (int idx = tid; idx < kChessBH * (kChessBS / 4); idx += kChessThreads) {
        const int r = idx / (kChessBS / 4), c = 4 * (idx - r * (kChessBS / 4));
        int h[3][4];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const unsigned lo = *reinterpret_cast<const unsigned*>(&s_gray[r + k][c]);
            const unsigned hi = *reinterpret_cast<const unsigned*>(&s_gray[r + k][c + 4]);
            const int g[6] = {(int)(lo & 255u), (int)((lo >> 8) & 255u), (int)((lo >> 16) & 255u), (int)(lo >> 24),
                              (int)(hi & 255u), (int)((hi >> 8) & 255u)};
#pragma unroll
            for (int j = 0; j < 4; ++j) h[k][j] = g[j] + 2 * g[j + 1] + g[j + 2];
        }
        unsigned v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = (unsigned)(h[0][j] + 2 * h[1][j] + h[2][j]);
        *reinterpret_cast<uint2*>(&s_blur[r][c]) = make_uint2(v[0] | (v[1] << 16), v[2] | (v[3] << 16));
    }
    __syncthreads();
    constexpr int ox[16] = {5, 5, 4, 2, 0, -2, -4, -5, -5, -5, -4, -2, 0, 2, 4, 5};
    constexpr int oy[16] = {0, 2, 4, 5, 5, 5, 4, 2, 0, -2, -4, -5, -5, -5, -4, -2};
    const int tx = tid & 63, ty = tid >> 6;
    const int px = (int)blockIdx.x * kChessTW + tx;
    int best = 0;
#pragma unroll
    for (int k = 0; k < kChessTH / kChessWaves; ++k) {
        const int row = ty + k * kChessWaves, py = (int)blockIdx.y * kChessTH + row;
        if (px >= W || py >= H) continue;
        int R = 0;
        if (px >= kChessHalo && px < W - kChessHalo && py >= kChessHalo && py < H - kChessHalo) {
            const int bc = tx + 5, br = row + 5;   // this pixel in the blur tile
            int I[16], sum = 0;
#pragma unroll
            for (int n = 0; n < 16; ++n) {
                I[n] = s_blur[br + oy[n]][bc + ox[n]];
                sum += I[n];
            }
            int sr = 0, dr = 0;
#pragma unroll
            for (int n = 0; n < 4; ++n) sr += abs(I[n] + I[n + 8] - I[n + 4] - I[n + 12]);
#pragma unroll
            for (int n = 0; n < 8; ++n) dr += abs(I[n] - I[n + 8]);
            const int c5 = s_blur[br][bc] + s_blur[br][bc - 1] + s_blur[br][bc + 1] + s_blur[br - 1][bc] + s_blur[br + 1][bc];
            R = 5 * (sr - dr) - abs(5 * sum - 16 * c5);
        }
        resp[f * H * W + (long)py * W + px] = R;
        best = max(best, R);
    }
    best = wave_max_i32(best);
    if (tx == 0 && best > 0) atomicMax(&rmax[f], best);
}

// rules 4: threshold, then the maximum of the (2 r + 1)^2 window clipped to the frame, ties to the earlier pixel
__device__ inline bool chess_candidate(const int* __restrict__ R, int H, int W, int i, int r, int t, int rmax) {
    const int v = R[i];
    if (v <= 0 || !(256LL * v > (long long)t * rmax)) return false;
    const int y = i / W, x = i - y * W;
    const int ya = max(y - r, 0), yb = min(y + r, H - 1), xa = max(x - r, 0), xb = min(x + r, W - 1);
    for (int yy = ya; yy <= yb; ++yy)
        for (int xx = xa; xx <= xb; ++xx) {
            const int j = yy * W + xx, q = R[j];
            if (j < i ? !(v > q) : !(v >= q)) return false;
        }
    return true;
}

// ---- launch 2: candidates per workgroup of kChessTile consecutive pixels; grid (groups, frames) ----
__global__ __launch_bounds__(kChessThreads) void chess_count_kernel(const int* __restrict__ resp, const int* __restrict__ rmax, int H,
                                                                    int W, int r, int t, unsigned* __restrict__ block_count) {
    __shared__ unsigned s_cnt;
    const long f = blockIdx.y, g = blockIdx.x;
    const int n = H * W;
    const int* R = resp + f * n;
    const int top = rmax[f];
    const long beg = g * kChessTile, end = min(beg + kChessTile, (long)n);
    const unsigned cnt = tile_count<kChessThreads>(beg, end, s_cnt, [&](long i) { return chess_candidate(R, H, W, (int)i, r, t, top); });
    if (threadIdx.x == 0) block_count[f * gridDim.x + g] = cnt;
}

// ---- launch 3: the counts become offsets; candidates are written in pixel order, the rest of the rows is padded ----
__global__ __launch_bounds__(kChessThreads) void chess_write_kernel(const int* __restrict__ resp, const int* __restrict__ rmax, int H,
                                                                    int W, int r, int t, const unsigned* __restrict__ block_count,
                                                                    int cap, int* __restrict__ xy, int* __restrict__ response,
                                                                    int* __restrict__ count) {
    __shared__ unsigned s_total, s_offset;
    __shared__ unsigned s_wtot[2][kChessWaves];
    const int tid = threadIdx.x;
    const long f = blockIdx.y, g = blockIdx.x;
    const int n = H * W;
    const int* R = resp + f * n;
    const int top = rmax[f];
    const unsigned* bc = block_count + f * gridDim.x;
    group_offsets<kChessThreads>(bc, (int)gridDim.x, g, s_total, s_offset);
    const unsigned total = s_total;
    int* oxy = xy + f * cap * 2;
    int* ore = response + f * cap;
    if (g == 0) {
        if (tid == 0) count[f] = (int)total;   // uncapped: an overflow is visible
        for (long k = (long)total + tid; k < cap; k += kChessThreads) {
            oxy[2 * k] = -1;
            oxy[2 * k + 1] = -1;
            ore[k] = 0;
        }
    }
    if (bc[g] == 0) return;   // uniform: nothing of this workgroup's to write
    const long beg = g * kChessTile, end = min(beg + kChessTile, (long)n);
    ordered_write<kChessThreads>(
        beg, end, (long)s_offset, s_wtot, [&](long i) { return chess_candidate(R, H, W, (int)i, r, t, top); },
        [&](long i, long row) {
            if (row < cap) {
                const int y = (int)i / W;
                oxy[2 * row] = (int)i - y * W;
                oxy[2 * row + 1] = y;
                ore[row] = R[i];
            }
        });
}

// ---- the refinement: one wave a point, four points a workgroup ----
__global__ __launch_bounds__(kChessThreads) void corner_subpix_kernel(const unsigned char* __restrict__ frames, int H, int W, int ch,
                                                                      const double* __restrict__ pin, const int* __restrict__ count,
                                                                      long total, int M, int wx, int wy, int iters,
                                                                      double* __restrict__ pout, unsigned char* __restrict__ ok) {
    __shared__ double s_patch[kChessWaves][kSubpixPatch * kSubpixPatch];
    __shared__ unsigned char s_foot[kChessWaves][kSubpixFoot * kSubpixFoot + 4];
    __shared__ double s_mx[2 * SKIMI_SUBPIX_MAX_WIN + 1], s_my[2 * SKIMI_SUBPIX_MAX_WIN + 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nx = 2 * wx + 1, ny = 2 * wy + 1, pw = nx + 2, ph = ny + 2, fw = pw + 1, fh = ph + 1;
    if (tid < nx) {
        const double u = (double)(tid - wx) / (double)wx;
        s_mx[tid] = exp(-(u * u));
    }
    if (tid >= 64 && tid - 64 < ny) {
        const double u = (double)(tid - 64 - wy) / (double)wy;
        s_my[tid - 64] = exp(-(u * u));
    }
    const long p = (long)blockIdx.x * kChessWaves + wave;
    const bool live = p < total;
    double x0 = 0.0, y0 = 0.0;
    bool started = false;
    const unsigned char* fp = frames;
    if (live) {
        const long f = p / M;
        x0 = pin[2 * p];
        y0 = pin[2 * p + 1];
        fp = frames + f * H * W * ch;
        started = (!count || (int)(p - f * M) < count[f]) && x0 >= 0.0 && x0 < (double)W && y0 >= 0.0 && y0 < (double)H;
    }
    double x = x0, y = y0;
    bool moving = started;                 // the same in every lane of the wave
    unsigned char* foot = s_foot[wave];
    double* patch = s_patch[wave];
    __syncthreads();
    for (int it = 0; it < iters; ++it) {   // every wave runs every round: the barriers are uniform
        double a = 0.0, b = 0.0;
        if (moving) {
            const double fx = floor(x), fy = floor(y);
            a = x - fx;
            b = y - fy;
            const int ix = (int)fx - wx - 1, iy = (int)fy - wy - 1;
            for (int k = lane; k < fw * fh; k += 64) {
                const int r = k / fw, c = k - r * fw;
                const int gx = min(max(ix + c, 0), W - 1), gy = min(max(iy + r, 0), H - 1);   // replicated border
                foot[k] = (unsigned char)chess_gray(fp + ((long)gy * W + gx) * ch, ch);
            }
        }
        __syncthreads();
        if (moving) {
            for (int k = lane; k < pw * ph; k += 64) {
                const int r = k / pw, c = k - r * pw;
                const unsigned char* q = foot + r * fw + c;
                const double p00 = q[0], p01 = q[1], p10 = q[fw], p11 = q[fw + 1];
                patch[k] = (1.0 - b) * ((1.0 - a) * p00 + a * p01) + b * ((1.0 - a) * p10 + a * p11);
            }
        }
        __syncthreads();
        if (moving) {
            double sa = 0.0, sb = 0.0, sc = 0.0, s1 = 0.0, s2 = 0.0;
            for (int k = lane; k < nx * ny; k += 64) {
                const int i = k / nx, j = k - i * nx;
                const double gx = patch[(i + 1) * pw + j + 2] - patch[(i + 1) * pw + j];
                const double gy = patch[(i + 2) * pw + j + 1] - patch[i * pw + j + 1];
                const double m = s_mx[j] * s_my[i];
                const double gxx = (gx * gx) * m, gxy = (gx * gy) * m, gyy = (gy * gy) * m;
                const double qx = (double)(j - wx), qy = (double)(i - wy);
                sa += gxx;
                sb += gxy;
                sc += gyy;
                s1 += gxx * qx + gxy * qy;
                s2 += gxy * qx + gyy * qy;
            }
            sa = wave_sum(sa);
            sb = wave_sum(sb);
            sc = wave_sum(sc);
            s1 = wave_sum(s1);
            s2 = wave_sum(s2);
            const double det = sa * sc - sb * sb;
            if (det == 0.0 || !isfinite(det)) {
                moving = false;            // a flat or degenerate patch: the point stays
            } else {
                x += (sc * s1 - sb * s2) / det;
                y += (sa * s2 - sb * s1) / det;
                if (!(x >= 0.0 && x < (double)W && y >= 0.0 && y < (double)H)) moving = false;   // left the frame (cv2 stops too)
            }
        }
    }
    if (live && lane == 0) {
        const bool good = started && fabs(x - x0) <= (double)wx && fabs(y - y0) <= (double)wy;   // a NaN fails
        pout[2 * p] = good ? x : x0;
        pout[2 * p + 1] = good ? y : y0;
        ok[p] = good ? 1 : 0;
    }
}

static inline long chess_groups(long n) { return cdiv(n, kChessTile); }
static inline bool chess_frame_ok(int64_t N, int32_t H, int32_t W) {
    return N >= 1 && N <= 65535 && H >= 1 && W >= 1 && H <= SKIMI_LENS_MAX_SIDE && W <= SKIMI_LENS_MAX_SIDE &&
           (int64_t)H * W <= SKIMI_CHESS_MAX_PIXELS;
}

}  // namespace skimi

using namespace skimi;

extern "C" {

size_t skimi_chess_workspace_bytes(int64_t N, int32_t H, int32_t W) {
    if (!chess_frame_ok(N, H, W)) return 0;
    const size_t n = (size_t)H * W;
    return align_up((size_t)N * n * 4 + (size_t)N * chess_groups((long)n) * 4, 8);
}

int skimi_chess_candidates(const uint8_t* frames, int64_t N, int32_t H, int32_t W, int32_t ch, int32_t threshold, int32_t nms_radius,
                           int32_t max_candidates, int32_t* xy, int32_t* response, int32_t* count, int32_t* rmax, void* ws,
                           size_t ws_bytes, void* stream) {
    SKIMI_CHECK_ARG(frames && xy && response && count && rmax && ws, "skimi_chess_candidates: null pointer");
    SKIMI_CHECK_ARG(chess_frame_ok(N, H, W),
                    "skimi_chess_candidates: need 1 <= N <= 65535 frames with sides in 1 .. %d and at most %d pixels (N = %lld, H = %d, W = %d)",
                    SKIMI_LENS_MAX_SIDE, SKIMI_CHESS_MAX_PIXELS, (long long)N, H, W);
    SKIMI_CHECK_ARG(ch == 1 || ch == 3 || ch == 4, "skimi_chess_candidates: 1, 3 or 4 channels, got %d", ch);
    SKIMI_CHECK_ARG(threshold >= 0 && threshold <= 256, "skimi_chess_candidates: threshold must be in 0 .. 256 (1/256 units), got %d", threshold);
    SKIMI_CHECK_ARG(nms_radius >= 0 && nms_radius <= SKIMI_CHESS_MAX_NMS, "skimi_chess_candidates: nms_radius must be in 0 .. %d, got %d",
                    SKIMI_CHESS_MAX_NMS, nms_radius);
    SKIMI_CHECK_ARG(max_candidates >= 1 && (int64_t)N * max_candidates <= (1LL << 30),
                    "skimi_chess_candidates: max_candidates must be >= 1 with N max_candidates <= 2^30, got %d", max_candidates);
    SKIMI_CHECK_ARG(ws_bytes >= skimi_chess_workspace_bytes(N, H, W), "skimi_chess_candidates: workspace too small (%zu < %zu bytes)",
                    ws_bytes, skimi_chess_workspace_bytes(N, H, W));
    SKIMI_CHECK_ARG(((uintptr_t)ws & 7) == 0, "skimi_chess_candidates: workspace must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const long n = (long)H * W, groups = chess_groups(n);
    int* resp = static_cast<int*>(ws);
    unsigned* block_count = reinterpret_cast<unsigned*>(resp + (size_t)N * n);
    SKIMI_HIP(hipMemsetAsync(rmax, 0, (size_t)N * 4, st));
    const dim3 block(kChessThreads), tiles((unsigned)cdiv(W, kChessTW), (unsigned)cdiv(H, kChessTH), (unsigned)N);
    if (ch == 1)
        hipLaunchKernelGGL(chess_response_kernel<1>, tiles, block, 0, st, frames, H, W, resp, rmax);
    else if (ch == 3)
        hipLaunchKernelGGL(chess_response_kernel<3>, tiles, block, 0, st, frames, H, W, resp, rmax);
    else
        hipLaunchKernelGGL(chess_response_kernel<4>, tiles, block, 0, st, frames, H, W, resp, rmax);
    const dim3 grid((unsigned)groups, (unsigned)N);
    hipLaunchKernelGGL(chess_count_kernel, grid, block, 0, st, (const int*)resp, (const int*)rmax, H, W, nms_radius, threshold, block_count);
    hipLaunchKernelGGL(chess_write_kernel, grid, block, 0, st, (const int*)resp, (const int*)rmax, H, W, nms_radius, threshold,
                       (const unsigned*)block_count, max_candidates, xy, response, count);
    SKIMI_LAUNCH_CHECK();
    return SKIMI_OK;
}

int skimi_corner_subpix(const uint8_t* frames, int64_t N, int32_t H, int32_t W, int32_t ch, const double* points, const int32_t* count,
                        int32_t M, int32_t win_x, int32_t win_y, int32_t iters, double* out, uint8_t* ok, void* stream) {
    SKIMI_CHECK_ARG(frames && points && out && ok, "skimi_corner_subpix: null pointer");
    SKIMI_CHECK_ARG(chess_frame_ok(N, H, W),
                    "skimi_corner_subpix: need 1 <= N <= 65535 frames with sides in 1 .. %d and at most %d pixels (N = %lld, H = %d, W = %d)",
                    SKIMI_LENS_MAX_SIDE, SKIMI_CHESS_MAX_PIXELS, (long long)N, H, W);
    SKIMI_CHECK_ARG(ch == 1 || ch == 3 || ch == 4, "skimi_corner_subpix: 1, 3 or 4 channels, got %d", ch);
    SKIMI_CHECK_ARG(M >= 0 && (int64_t)N * M <= (1LL << 30), "skimi_corner_subpix: need M >= 0 points a frame with N M <= 2^30, got %d", M);
    SKIMI_CHECK_ARG(win_x >= 1 && win_x <= SKIMI_SUBPIX_MAX_WIN && win_y >= 1 && win_y <= SKIMI_SUBPIX_MAX_WIN,
                    "skimi_corner_subpix: the half window must be in 1 .. %d each way, got (%d, %d)", SKIMI_SUBPIX_MAX_WIN, win_x, win_y);
    SKIMI_CHECK_ARG(iters >= 0 && iters <= SKIMI_SUBPIX_MAX_ITERS, "skimi_corner_subpix: iters must be in 0 .. %d, got %d",
                    SKIMI_SUBPIX_MAX_ITERS, iters);
    const long total = (long)N * M;
    if (total == 0) return SKIMI_OK;
    hipLaunchKernelGGL(corner_subpix_kernel, dim3((unsigned)cdiv(total, kChessWaves)), dim3(kChessThreads), 0, (hipStream_t)stream, frames, H,
                       W, ch, points, count, total, M, win_x, win_y, iters, out, ok);
    SKIMI_LAUNCH_CHECK();
    return SKIMI_OK;
}

}  // extern "C"
