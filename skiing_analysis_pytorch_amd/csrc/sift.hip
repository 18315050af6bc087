// SIFT-style image features on whole frames and a brute-force L2 matcher with Lowe's ratio test (camera_position.py:120-178,
// 242-297: estimate_camera_pose_from_SIFT, estimate_pose_from_bbox_region = cv2.SIFT_create + BFMatcher.knnMatch + ratio test)
// under the project's own rules: DESIGN §2 "Image features (SIFT-style)", the block in include/skimi.h; tests/sift_restated.py
// evaluates the same expressions.
//   blur, half           the Gaussian scale space in float32: one launch a (octave, layer) for all frames; a 64 x 32 tile with
//                        its halo in LDS, the horizontal pass into a second LDS tile, the vertical pass out of it.  The first
//                        launch reads the frame's bytes through features.hip's gray.  Taps come from the host.
//   count / write        compact.h's exact compaction in (octave, layer, y, x) order of the 26-neighbour extrema of the
//                        difference of neighbouring layers (computed where it is read, never stored)
//   refine               a candidate a lane: the quadratic fit in float64 with + - * / only, contrast and edge tests, the box
//   select               one workgroup a frame: compact.h's exact radix selection of the M largest |response|, ties to
//                        the earlier candidate, rows in candidate order
//   describe             one wave a keypoint: the orientation histogram and the 4 x 4 x 8 descriptor in float64, votes added
//                        in LDS as integers of unit 2^-43, so the sums do not depend on the order of the lanes
//   l2_nn, l2_keep       the matcher: nearest and second-nearest train rows on a grid of (64 queries, pair of sets, direction)
//                        with v_dot4_u32_u8 on the bytes, then one workgroup a pair for the keep rule and a stable LDS radix
//                        sort of the kept pairs by (distance, query)
#include <algorithm>

#include "common.h"
#include "compact.h"
#include "gray.h"
#include "reduce.h"

namespace skimi {

constexpr int kSiftThreads = 256;
constexpr int kSiftWaves = kSiftThreads / 64;
constexpr int kSiftS = 3, kSiftLayers = kSiftS + 3;
constexpr int kSiftR = SKIMI_SIFT_MAX_RADIUS;
constexpr int kSiftTaps = 2 * kSiftR + 1;
constexpr int kBlurTW = 64, kBlurTH = 32;
constexpr int kBlurSW = kBlurTW + 2 * kSiftR, kBlurSH = kBlurTH + 2 * kSiftR;   // 90 x 58
constexpr int kBlurSS = kBlurSW + 1;                                          // floats of a source row in LDS
constexpr long kSiftTile = 4096;              // pixels of a workgroup of the candidate launches
constexpr int kSiftSegs = kSiftS * SKIMI_SIFT_MAX_OCTAVES;
constexpr int kSiftB = SKIMI_SIFT_BORDER;
constexpr int kSiftMaxM = SKIMI_SIFT_MAX_FEATURES;
constexpr double kVoteUnit = 8796093022208.0;  // 2^43
constexpr double kTwoPi = 6.283185307179586;

// the octaves of one frame and where each starts in the per-frame arrays of the workspace; segment s = 3 o + (layer - 1)
struct SiftPyr {
    int O, Oe, M;                             // requested octaves, those that are not empty, max_features
    int W[SKIMI_SIFT_MAX_OCTAVES], H[SKIMI_SIFT_MAX_OCTAVES], cap[SKIMI_SIFT_MAX_OCTAVES];
    long poff[SKIMI_SIFT_MAX_OCTAVES];        // floats ahead of the octave's six planes
    long coff[kSiftSegs], goff[kSiftSegs];
    long P, C, G;                             // floats, candidate rows and candidate workgroups of a frame
};

struct SiftWs {
    float* gauss;                             // [N, P]
    int* cand;                                // [N, C] pixel index in its octave
    unsigned* block_count;                    // [N, G]
    int* seg_count;                           // [N, kSiftSegs]
    unsigned long long* key;                  // [N, C] bits of |response|, 0: dropped
    double* rxy;                              // [N, C, 2]
    double* rsr;                              // [N, C, 2] sigma, response
    int* rpos;                                // [N, C, 4] x, y, layer, 0
};

// ---- the scale space ----
template <int SRC>
__device__ __forceinline__ float sift_src(const void* __restrict__ src, long i) {
    if (SRC == 0) return static_cast<const float*>(src)[i];
    return (float)orb_gray<(SRC == 0 ? 1 : SRC)>(static_cast<const unsigned char*>(src) + i * SRC);
}

// grid (tiles, frames).  SRC 0: an f32 plane, `sstride` floats a frame; 1, 3, 4: the u8 frames with SRC channels
template <int SRC>
__global__ __launch_bounds__(kSiftThreads) void sift_blur_kernel(const void* __restrict__ src, long sstride, float* __restrict__ dst,
                                                                 long dstride, int W, int H, const float* __restrict__ taps, int r) {
    __shared__ float s_src[kBlurSH][kBlurSS];
    __shared__ float s_mid[kBlurSH][kBlurTW];
    __shared__ float s_tap[kSiftTaps];
    const int tid = threadIdx.x, tx = tid & 63, wv = tid >> 6;
    const int tilesx = (W + kBlurTW - 1) / kBlurTW;
    const int bx = ((int)blockIdx.x % tilesx) * kBlurTW, by = ((int)blockIdx.x / tilesx) * kBlurTH;
    const long f = blockIdx.y;
    const int rows = kBlurTH + 2 * r, cols = kBlurTW + 2 * r, nt = 2 * r + 1;
    if (tid < nt) s_tap[tid] = taps[kSiftR - r + tid];
    const long base = SRC == 0 ? f * sstride : f * (long)W * H;
    for (int idx = tid; idx < rows * cols; idx += kSiftThreads) {
        const int rr = idx / cols, c = idx - rr * cols;
        const int gx = min(max(bx - r + c, 0), W - 1), gy = min(max(by - r + rr, 0), H - 1);
        s_src[rr][c] = sift_src<SRC>(src, base + (long)gy * W + gx);
    }
    __syncthreads();
    for (int rr = wv; rr < rows; rr += kSiftWaves) {
        float acc = s_tap[0] * s_src[rr][tx];
        for (int k = 1; k < nt; ++k) acc = acc + s_tap[k] * s_src[rr][tx + k];
        s_mid[rr][tx] = acc;
    }
    __syncthreads();
    const int px = bx + tx;
    float* out = dst + f * dstride;
    for (int ty = wv; ty < kBlurTH; ty += kSiftWaves) {
        const int py = by + ty;
        if (px >= W || py >= H) continue;
        float acc = s_tap[0] * s_mid[ty][tx];
        for (int k = 1; k < nt; ++k) acc = acc + s_tap[k] * s_mid[ty + k][tx];
        out[(long)py * W + px] = acc;
    }
}

// layer 0 of an octave: the even pixels of layer S of the octave before
__global__ __launch_bounds__(kSiftThreads) void sift_half_kernel(const float* __restrict__ src, float* __restrict__ dst, long stride, int Ws,
                                                                 int Wd, int Hd) {
    const long f = blockIdx.y, i = (long)blockIdx.x * kSiftThreads + threadIdx.x;
    if (i >= (long)Wd * Hd) return;
    const int y = (int)(i / Wd), x = (int)(i - (long)y * Wd);
    dst[f * stride + i] = src[f * stride + (long)(2 * y) * Ws + 2 * x];
}

// ---- candidates ----
// DoG layer l of an octave at pixel index i: Gaussian layer l + 1 - layer l in f32
__device__ __forceinline__ float sift_dog(const float* __restrict__ G, long plane, int l, long i) {
    return G[(long)(l + 1) * plane + i] - G[(long)l * plane + i];
}

__device__ inline bool sift_candidate(const float* __restrict__ G, int W, int H, int l, int i) {
    const int y = i / W, x = i - y * W;
    if (x < kSiftB || x >= W - kSiftB || y < kSiftB || y >= H - kSiftB) return false;
    const long plane = (long)W * H;
    const float d = sift_dog(G, plane, l, i);
    if (!(fabsf(d) > SKIMI_SIFT_PRETHRESH)) return false;
    bool mx = true, mn = true;
    for (int dl = -1; dl <= 1; ++dl) {
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                if (dl == 0 && dy == 0 && dx == 0) continue;
                const float q = sift_dog(G, plane, l + dl, (long)i + dy * W + dx);
                mx = mx && d > q;
                mn = mn && d < q;
            }
        if (!mx && !mn) return false;
    }
    return mx || mn;
}

// grid (groups of octave 0, 3 Oe, frames)
__global__ __launch_bounds__(kSiftThreads) void sift_count_kernel(SiftPyr py, const float* __restrict__ gauss,
                                                                  unsigned* __restrict__ block_count) {
    __shared__ unsigned s_cnt;
    const int s = blockIdx.y, o = s / kSiftS, l = s - o * kSiftS + 1, W = py.W[o], H = py.H[o];
    const long n = (long)W * H, g = blockIdx.x, f = blockIdx.z;
    if (g * kSiftTile >= n) return;
    const float* G = gauss + f * py.P + py.poff[o];
    const long beg = g * kSiftTile, end = min(beg + kSiftTile, n);
    const unsigned cnt = tile_count<kSiftThreads>(beg, end, s_cnt, [&](long i) { return sift_candidate(G, W, H, l, (int)i); });
    if (threadIdx.x == 0) block_count[f * py.G + py.goff[s] + g] = cnt;
}

__global__ __launch_bounds__(kSiftThreads) void sift_write_kernel(SiftPyr py, const float* __restrict__ gauss,
                                                                  const unsigned* __restrict__ block_count, int* __restrict__ cand,
                                                                  int* __restrict__ seg_count) {
    __shared__ unsigned s_total, s_offset;
    __shared__ unsigned s_wtot[2][kSiftWaves];
    const int s = blockIdx.y, o = s / kSiftS, l = s - o * kSiftS + 1, W = py.W[o], H = py.H[o];
    const long n = (long)W * H, g = blockIdx.x, f = blockIdx.z;
    if (g * kSiftTile >= n) return;
    const int groups = (int)((n + kSiftTile - 1) / kSiftTile);
    const float* G = gauss + f * py.P + py.poff[o];
    const unsigned* bc = block_count + f * py.G + py.goff[s];
    group_offsets<kSiftThreads>(bc, groups, g, s_total, s_offset);
    if (g == 0 && threadIdx.x == 0) seg_count[f * kSiftSegs + s] = (int)s_total;
    if (bc[g] == 0) return;                   // uniform
    int* oc = cand + f * py.C + py.coff[s];
    const long cap = py.cap[o];
    const long beg = g * kSiftTile, end = min(beg + kSiftTile, n);
    ordered_write<kSiftThreads>(
        beg, end, (long)s_offset, s_wtot, [&](long i) { return sift_candidate(G, W, H, l, (int)i); },
        [&](long i, long row) {
            if (row < cap) oc[row] = (int)i;
        });
}

// ---- refinement (rule 4): f64, + - * / only ----
__device__ __forceinline__ double sift_D(const float* __restrict__ G, long plane, int W, int l, int y, int x) {
    return (double)sift_dog(G, plane, l, (long)y * W + x);
}

struct SiftRef {
    double X, Y, sigma, resp;
    int x, y, l;
    bool ok;
};

__device__ inline SiftRef sift_refine(const float* __restrict__ G, int W, int H, int o, int l, int x, int y, const double* __restrict__ box) {
    SiftRef out{};
    out.ok = false;
    const long plane = (long)W * H;
    double X0 = 0, X1 = 0, X2 = 0, g0 = 0, g1 = 0, g2 = 0, dxx = 0, dyy = 0, dxy = 0, v = 0;
    bool settled = false;
    for (int round = 0; round < 5; ++round) {
        v = sift_D(G, plane, W, l, y, x);
        g0 = (sift_D(G, plane, W, l, y, x + 1) - sift_D(G, plane, W, l, y, x - 1)) * 0.5;
        g1 = (sift_D(G, plane, W, l, y + 1, x) - sift_D(G, plane, W, l, y - 1, x)) * 0.5;
        g2 = (sift_D(G, plane, W, l + 1, y, x) - sift_D(G, plane, W, l - 1, y, x)) * 0.5;
        const double v2 = 2.0 * v;
        dxx = sift_D(G, plane, W, l, y, x + 1) + sift_D(G, plane, W, l, y, x - 1) - v2;
        dyy = sift_D(G, plane, W, l, y + 1, x) + sift_D(G, plane, W, l, y - 1, x) - v2;
        const double dss = sift_D(G, plane, W, l + 1, y, x) + sift_D(G, plane, W, l - 1, y, x) - v2;
        dxy = (sift_D(G, plane, W, l, y + 1, x + 1) - sift_D(G, plane, W, l, y + 1, x - 1) - sift_D(G, plane, W, l, y - 1, x + 1) +
               sift_D(G, plane, W, l, y - 1, x - 1)) * 0.25;
        const double dxs = (sift_D(G, plane, W, l + 1, y, x + 1) - sift_D(G, plane, W, l + 1, y, x - 1) - sift_D(G, plane, W, l - 1, y, x + 1) +
                            sift_D(G, plane, W, l - 1, y, x - 1)) * 0.25;
        const double dys = (sift_D(G, plane, W, l + 1, y + 1, x) - sift_D(G, plane, W, l + 1, y - 1, x) - sift_D(G, plane, W, l - 1, y + 1, x) +
                            sift_D(G, plane, W, l - 1, y - 1, x)) * 0.25;
        // [dxx dxy dxs; dxy dyy dys; dxs dys dss] X = -g, elimination without pivoting
        const double b0 = -g0, b1 = -g1, b2 = -g2;
        const double m10 = dxy / dxx, m20 = dxs / dxx;
        const double a11 = dyy - m10 * dxy, a12 = dys - m10 * dxs, c1 = b1 - m10 * b0;
        const double a21 = dys - m20 * dxy, a22 = dss - m20 * dxs, c2 = b2 - m20 * b0;
        const double m21 = a21 / a11;
        const double e22 = a22 - m21 * a12, e2 = c2 - m21 * c1;
        X2 = e2 / e22;
        X1 = (c1 - a12 * X2) / a11;
        X0 = (b0 - dxy * X1 - dxs * X2) / dxx;
        const int mx = X0 > 0.5 ? 1 : (X0 < -0.5 ? -1 : 0), my = X1 > 0.5 ? 1 : (X1 < -0.5 ? -1 : 0), ml = X2 > 0.5 ? 1 : (X2 < -0.5 ? -1 : 0);
        if (mx == 0 && my == 0 && ml == 0) {
            settled = true;
            break;
        }
        x += mx, y += my, l += ml;
        if (l < 1 || l > kSiftS || x < kSiftB || x >= W - kSiftB || y < kSiftB || y >= H - kSiftB) return out;
    }
    if (!settled) return out;
    const double resp = v + ((g0 * X0 + g1 * X1) + g2 * X2) * 0.5;
    const double tr = dxx + dyy, det = dxx * dyy - dxy * dxy;
    if (!(fabs(resp) >= SKIMI_SIFT_CONTRAST) || !(det > 0.0) || !(tr * tr * 10.0 < 121.0 * det)) return out;
    const double scale = (double)(1 << o);
    out.X = ((double)x + X0) * scale;
    out.Y = ((double)y + X1) * scale;
    const double z = (((double)l + X2) / 3.0 - 2.0 / 3.0) * SKIMI_SIFT_LN2;
    double p = 1.0;
    for (int k = 16; k >= 1; --k) p = 1.0 + z * p / (double)k;
    out.sigma = 1.6 * scale * SKIMI_SIFT_CBRT4 * p;
    out.resp = resp;
    out.x = x, out.y = y, out.l = l;
    out.ok = !box || (out.X >= box[0] && out.X < box[2] && out.Y >= box[1] && out.Y < box[3]);
    return out;
}

// grid (rows of the largest capacity / threads, 3 Oe, frames)
__global__ __launch_bounds__(kSiftThreads) void sift_refine_kernel(SiftPyr py, const float* __restrict__ gauss, const int* __restrict__ cand,
                                                                   const int* __restrict__ seg_count, const double* __restrict__ roi,
                                                                   unsigned long long* __restrict__ key, double* __restrict__ rxy,
                                                                   double* __restrict__ rsr, int* __restrict__ rpos) {
    const int s = blockIdx.y, o = s / kSiftS, l = s - o * kSiftS + 1, W = py.W[o], H = py.H[o];
    const long f = blockIdx.z, r = (long)blockIdx.x * kSiftThreads + threadIdx.x;
    if (r >= min(seg_count[f * kSiftSegs + s], py.cap[o])) return;
    const long c = f * py.C + py.coff[s] + r;
    const int p = cand[c], y = p / W, x = p - y * W;
    const SiftRef ref = sift_refine(gauss + f * py.P + py.poff[o], W, H, o, l, x, y, roi ? roi + 4 * f : nullptr);
    key[c] = ref.ok ? (unsigned long long)__double_as_longlong(fabs(ref.resp)) : 0ull;
    if (ref.ok) {
        rxy[2 * c] = ref.X;
        rxy[2 * c + 1] = ref.Y;
        rsr[2 * c] = ref.sigma;
        rsr[2 * c + 1] = ref.resp;
        rpos[4 * c] = ref.x;
        rpos[4 * c + 1] = ref.y;
        rpos[4 * c + 2] = ref.l;
        rpos[4 * c + 3] = 0;
    }
}

// ---- selection (rule 5): grid (frames) ----
__global__ __launch_bounds__(kSiftThreads) void sift_select_kernel(SiftPyr py, const int* __restrict__ seg_count,
                                                                   const unsigned long long* __restrict__ key, const double* __restrict__ rxy,
                                                                   const double* __restrict__ rsr, const int* __restrict__ rpos,
                                                                   double* __restrict__ xy, int* __restrict__ xy_level, int* __restrict__ octave,
                                                                   int* __restrict__ layer, double* __restrict__ sigma, double* __restrict__ response,
                                                                   double* __restrict__ angle, unsigned char* __restrict__ desc,
                                                                   int* __restrict__ count, int* __restrict__ octave_count) {
    __shared__ unsigned s_hist[256];
    __shared__ unsigned s_digit, s_need;
    __shared__ unsigned s_wtot[2][2][kSiftWaves];
    __shared__ int s_n[kSiftSegs];
    const int M = py.M, tid = threadIdx.x, segs = kSiftS * py.Oe;
    const long f = blockIdx.x;
    if (tid < kSiftSegs) s_n[tid] = tid < segs ? min(seg_count[f * kSiftSegs + tid], py.cap[tid / kSiftS]) : 0;
    if (tid < py.O) {
        int c = 0;
        if (tid < py.Oe)
            for (int k = 0; k < kSiftS; ++k) c += seg_count[f * kSiftSegs + kSiftS * tid + k];
        octave_count[f * py.O + tid] = c;
    }
    __syncthreads();
    long rows = 0;
    for (int s = 0; s < segs; ++s) rows += s_n[s];
    const unsigned long long* kf = key + f * py.C;
    // the key T of descending rank M - 1 and how many of the keys equal to it are kept; rows <= M keeps every key > 0
    unsigned long long T = 0;
    unsigned need = 0;
    if (rows > M)
        select_threshold<kSiftThreads>(
            (unsigned)M,
            [&](auto&& add) {
                for (int s = 0; s < segs; ++s) {
                    const unsigned long long* ks = kf + py.coff[s];
                    for (int i = tid; i < s_n[s]; i += kSiftThreads) add(ks[i]);
                }
            },
            s_hist, s_digit, s_need, T, need);
    long row0 = 0;
    unsigned eq0 = 0;
    int buf = 0;
    for (int s = 0; s < segs; ++s) {
        const int n = s_n[s], o = s / kSiftS;
        const long cb = f * py.C + py.coff[s];
        for (int i0 = 0; i0 < n; i0 += kSiftThreads) {       // uniform trip count
            const int i = i0 + tid;
            const bool live = i < n;
            const unsigned long long k = live ? key[cb + i] : 0;
            unsigned rank, chunk;
            if (select_rank<kSiftWaves>(k, live && k > 0, rows > M, T, need, eq0, s_wtot[buf], rank, chunk)) {
                const long r = row0 + rank;
                if (r < M) {
                    const long q = f * M + r, c = cb + i;
                    xy[2 * q] = rxy[2 * c];
                    xy[2 * q + 1] = rxy[2 * c + 1];
                    xy_level[2 * q] = rpos[4 * c];
                    xy_level[2 * q + 1] = rpos[4 * c + 1];
                    octave[q] = o;
                    layer[q] = rpos[4 * c + 2];
                    sigma[q] = rsr[2 * c];
                    response[q] = rsr[2 * c + 1];
                }
            }
            row0 += chunk;
            buf ^= 1;
        }
    }
    const long total = min(row0, (long)M);
    if (tid == 0) count[f] = (int)total;
    for (long r = total + tid; r < M; r += kSiftThreads) {
        const long q = f * M + r;
        xy[2 * q] = xy[2 * q + 1] = -1.0;
        xy_level[2 * q] = xy_level[2 * q + 1] = -1;
        octave[q] = layer[q] = -1;
        sigma[q] = response[q] = 0.0;
        angle[q] = -1.0;
        uint4* d = reinterpret_cast<uint4*>(desc + 128 * q);
#pragma unroll
        for (int w = 0; w < 8; ++w) d[w] = make_uint4(0, 0, 0, 0);
    }
}

// ---- orientation and descriptor (rules 6, 7): one wave a row; every wave meets every barrier ----
__device__ __forceinline__ double sift_smooth(const double* h, int k) {
    return ((h[(k + 34) % 36] + h[(k + 2) % 36]) + 4.0 * (h[(k + 35) % 36] + h[(k + 1) % 36]) + 6.0 * h[k]) / 16.0;
}

__device__ __forceinline__ void sift_vote(unsigned long long* bin, double v) {
    atomicAdd(bin, (unsigned long long)__double2ll_rn(v * kVoteUnit));
}

__global__ __launch_bounds__(kSiftThreads) void sift_describe_kernel(SiftPyr py, const float* __restrict__ gauss, const int* __restrict__ xy_level,
                                                                     const int* __restrict__ octave, const int* __restrict__ layer,
                                                                     const double* __restrict__ sigma, const int* __restrict__ count, long total,
                                                                     double* __restrict__ angle, unsigned char* __restrict__ desc) {
    __shared__ unsigned long long s_bins[kSiftWaves][128];
    __shared__ double s_h[kSiftWaves][2][36];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long q = (long)blockIdx.x * kSiftWaves + wave;
    const long f = q < total ? q / py.M : 0;
    const bool valid = q < total && (int)(q - f * py.M) < count[f];
    int W = 1, H = 1, x = 0, y = 0;
    double s = 0.0;
    const float* L = gauss;
    if (valid) {
        const int o = octave[q];
        W = py.W[o], H = py.H[o], x = xy_level[2 * q], y = xy_level[2 * q + 1];
        s = sigma[q] / (double)(1 << o);
        L = gauss + f * py.P + py.poff[o] + (long)layer[q] * W * H;
    }
    unsigned long long* bins = s_bins[wave];
    bins[lane] = 0;
    bins[lane + 64] = 0;
    __syncthreads();
    if (valid) {
        const double rad = 4.5 * s, rad2 = rad * rad, den = 2.0 * (1.5 * s) * (1.5 * s);
        const int R = (int)floor(rad), side = 2 * R + 1;
        for (int k = lane; k < side * side; k += 64) {
            const int i = k / side - R, j = k - (i + R) * side - R;
            const int px = x + j, pyx = y + i;
            if (px < 1 || px > W - 2 || pyx < 1 || pyx > H - 2 || (double)(i * i + j * j) > rad2) continue;
            const float* c = L + (long)pyx * W + px;
            const double gx = (double)c[1] - (double)c[-1], gy = (double)c[W] - (double)c[-W];
            const double w = sqrt(gx * gx + gy * gy) * exp(-(double)(i * i + j * j) / den);
            double th = atan2(gy, gx);
            if (th < 0.0) th += kTwoPi;
            const double fb = th * 36.0 / kTwoPi, b0 = floor(fb), fr = fb - b0;
            const int k0 = (int)b0 % 36, k1 = (k0 + 1) % 36;
            sift_vote(&bins[k0], w * (1.0 - fr));
            sift_vote(&bins[k1], w * fr);
        }
    }
    __syncthreads();
    if (lane < 36) s_h[wave][0][lane] = (double)(long long)bins[lane] / kVoteUnit;
    __syncthreads();
    if (lane < 36) s_h[wave][1][lane] = sift_smooth(s_h[wave][0], lane);
    __syncthreads();
    if (lane < 36) s_h[wave][0][lane] = sift_smooth(s_h[wave][1], lane);
    __syncthreads();
    double ang = 0.0;
    {
        const double* h = s_h[wave][0];
        int kb = 0;
        double top = h[0];
        for (int k = 1; k < 36; ++k)
            if (h[k] > top) {
                top = h[k];
                kb = k;
            }
        const double l = h[(kb + 35) % 36], r = h[(kb + 1) % 36], dn = l - 2.0 * top + r;
        const double p = (double)kb + (dn != 0.0 ? 0.5 * (l - r) / dn : 0.0);
        ang = kTwoPi * p / 36.0;
        if (ang < 0.0) ang += kTwoPi;
        if (ang >= kTwoPi) ang -= kTwoPi;
    }
    bins[lane] = 0;
    bins[lane + 64] = 0;
    __syncthreads();
    if (valid) {
        const double ca = cos(ang), sa = sin(ang), hw = 3.0 * s;
        const int R = (int)floor(hw * 1.4142135623730951 * 2.5 + 0.5), side = 2 * R + 1;
        for (int k = lane; k < side * side; k += 64) {
            const int i = k / side - R, j = k - (i + R) * side - R;
            const int px = x + j, pyx = y + i;
            if (px < 1 || px > W - 2 || pyx < 1 || pyx > H - 2) continue;
            const double cr = (ca * (double)j + sa * (double)i) / hw, rr = (-sa * (double)j + ca * (double)i) / hw;
            const double rb = rr + 1.5, cb = cr + 1.5;
            if (!(rb > -1.0 && rb < 4.0 && cb > -1.0 && cb < 4.0)) continue;
            const float* c = L + (long)pyx * W + px;
            const double gx = (double)c[1] - (double)c[-1], gy = (double)c[W] - (double)c[-W];
            double ob = (atan2(gy, gx) - ang) * 8.0 / kTwoPi;
            ob -= floor(ob / 8.0) * 8.0;
            const double val = sqrt(gx * gx + gy * gy) * exp(-(rr * rr + cr * cr) / 8.0);
            const double r0 = floor(rb), c0 = floor(cb), o0 = floor(ob);
            const double fr = rb - r0, fc = cb - c0, fo = ob - o0;
            const int ir = (int)r0, ic = (int)c0, io = (int)o0;
#pragma unroll
            for (int dr = 0; dr < 2; ++dr) {
                const int row = ir + dr;
                if (row < 0 || row > 3) continue;
                const double vr = val * (dr ? fr : 1.0 - fr);
#pragma unroll
                for (int dc = 0; dc < 2; ++dc) {
                    const int col = ic + dc;
                    if (col < 0 || col > 3) continue;
                    const double vc = vr * (dc ? fc : 1.0 - fc);
                    sift_vote(&bins[(row * 4 + col) * 8 + (io & 7)], vc * (1.0 - fo));
                    sift_vote(&bins[(row * 4 + col) * 8 + ((io + 1) & 7)], vc * fo);
                }
            }
        }
    }
    __syncthreads();
    double v0 = (double)(long long)bins[lane] / kVoteUnit, v1 = (double)(long long)bins[lane + 64] / kVoteUnit;
    double nrm = sqrt(wave_sum(v0 * v0 + v1 * v1));
    int b0 = 0, b1 = 0;
    if (nrm > 0.0) {
        v0 = fmin(v0 / nrm, 0.2);
        v1 = fmin(v1 / nrm, 0.2);
        nrm = sqrt(wave_sum(v0 * v0 + v1 * v1));
        b0 = min(255, (int)__double2ll_rn(512.0 * (v0 / nrm)));
        b1 = min(255, (int)__double2ll_rn(512.0 * (v1 / nrm)));
    }
    if (valid) {
        desc[128 * q + lane] = (unsigned char)b0;
        desc[128 * q + 64 + lane] = (unsigned char)b1;
        if (lane == 0) angle[q] = ang;
    }
}

// ---- the matcher (rule 8) ----
constexpr int kL2Q = 64;                      // queries of a workgroup: a query a lane, the four waves share the train tile
constexpr int kL2Tile = 64;                   // train descriptors staged at a time (8 KiB)
constexpr int kL2SortThreads = 1024;
constexpr unsigned long long kL2None = ~0ull;

__device__ __forceinline__ unsigned l2_dot16(const uint4& a, const uint4& b, unsigned acc) {
    acc = __builtin_amdgcn_udot4(a.x, b.x, acc, false);
    acc = __builtin_amdgcn_udot4(a.y, b.y, acc, false);
    acc = __builtin_amdgcn_udot4(a.z, b.z, acc, false);
    return __builtin_amdgcn_udot4(a.w, b.w, acc, false);
}

// grid (blocks of kL2Q queries, pairs of sets, 1 or 2 directions): direction 0 searches d2 for the rows of d1, 1 the reverse.
// best [.., M] = (distance << 12 | train index) of the nearest, second [.., M1] = the second distance (-1: none; direction 0)
__global__ __launch_bounds__(kSiftThreads) void l2_nn_kernel(const unsigned char* __restrict__ d1, const int* __restrict__ n1, int M1,
                                                            const unsigned char* __restrict__ d2, const int* __restrict__ n2, int M2,
                                                            unsigned long long* __restrict__ best12, unsigned long long* __restrict__ best21,
                                                            int* __restrict__ second) {
    __shared__ uint4 s_row[kL2Tile][8];
    __shared__ unsigned s_norm[kL2Tile];
    __shared__ unsigned long long s_b[2][kSiftWaves][kL2Q];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, dir = blockIdx.z;
    const long b = blockIdx.y;
    const int na = min(max(n1[b], 0), M1), nb = min(max(n2[b], 0), M2);
    const int nq = dir ? nb : na, nt = dir ? na : nb, Mq = dir ? M2 : M1, Mt = dir ? M1 : M2;
    const int i = (int)blockIdx.x * kL2Q + lane;
    if ((int)blockIdx.x * kL2Q >= nq) return;
    const uint4* Q = reinterpret_cast<const uint4*>((dir ? d2 : d1) + (b * Mq + min(i, nq - 1)) * 128);
    const uint4* Tr = reinterpret_cast<const uint4*>((dir ? d1 : d2) + b * (long)Mt * 128);
    uint4 q[8];
    unsigned qn = 0;
#pragma unroll
    for (int w = 0; w < 8; ++w) {
        q[w] = Q[w];
        qn = l2_dot16(q[w], q[w], qn);
    }
    unsigned long long b1 = kL2None, b2 = kL2None;
    for (int t0 = 0; t0 < nt; t0 += kL2Tile) {
        const int cnt = min(kL2Tile, nt - t0);
        __syncthreads();
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int k = tid + h * kSiftThreads, row = k >> 3;   // eight consecutive lanes load a row
            uint4 v = make_uint4(0, 0, 0, 0);
            if (row < cnt) v = Tr[(long)(t0 + row) * 8 + (k & 7)];
            (&s_row[0][0])[k] = v;
            unsigned part = l2_dot16(v, v, 0);
            part += (unsigned)__shfl_xor((int)part, 1, 64);
            part += (unsigned)__shfl_xor((int)part, 2, 64);
            part += (unsigned)__shfl_xor((int)part, 4, 64);
            if ((k & 7) == 0) s_norm[row] = part;
        }
        __syncthreads();
        for (int j = wave; j < cnt; j += kSiftWaves) {
            unsigned dot = 0;
#pragma unroll
            for (int w = 0; w < 8; ++w) dot = l2_dot16(q[w], s_row[j][w], dot);
            const unsigned d = qn + s_norm[j] - 2u * dot;
            const unsigned long long key = ((unsigned long long)d << 12) | (unsigned)(t0 + j);
            b2 = min(b2, max(b1, key));
            b1 = min(b1, key);
        }
    }
    s_b[0][wave][lane] = b1;
    s_b[1][wave][lane] = b2;
    __syncthreads();
    if (wave == 0 && i < nq) {
#pragma unroll
        for (int w = 1; w < kSiftWaves; ++w) {
            const unsigned long long x1 = s_b[0][w][lane], x2 = s_b[1][w][lane];
            b2 = min(max(b1, x1), min(b2, x2));
            b1 = min(b1, x1);
        }
        if (dir)
            best21[b * M2 + i] = b1;
        else {
            best12[b * M1 + i] = b1;
            second[b * M1 + i] = b2 == kL2None ? -1 : (int)(b2 >> 12);
        }
    }
}

// One stable scatter step of the workgroup: wave w owns the positions 256 w .. 256 w + 255 in four rounds of 64.  digit[r]
// (0 .. 255, or -1: no element) of position 256 w + 64 r + lane -> its destination.  s_cnt [16][256], s_start [257].
__device__ inline void l2_scatter(const int (&digit)[4], unsigned (&dest)[4], unsigned (*s_cnt)[256], unsigned* s_start) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int k = tid; k < 16 * 256; k += kL2SortThreads) (&s_cnt[0][0])[k] = 0;
    __syncthreads();
    unsigned local[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int d = digit[r];
        unsigned long long m = __ballot(d >= 0);
#pragma unroll
        for (int bit = 0; bit < 8; ++bit) {
            const unsigned long long bb = __ballot((d >> bit) & 1);
            m &= ((d >> bit) & 1) ? bb : ~bb;
        }
        local[r] = 0;
        if (d >= 0) {
            const unsigned below = (unsigned)__popcll(m & ((1ull << lane) - 1ull));
            local[r] = s_cnt[wave][d] + below;
        }
        __syncthreads();                      // every lane of the wave has read the running count
        if (d >= 0 && (m & ((1ull << lane) - 1ull)) == 0) s_cnt[wave][d] += (unsigned)__popcll(m);
        __syncthreads();
    }
    if (tid < 256) {
        unsigned run = 0;
        for (int w = 0; w < 16; ++w) {
            const unsigned c = s_cnt[w][tid];
            s_cnt[w][tid] = run;
            run += c;
        }
        s_start[tid + 1] = run;
    }
    __syncthreads();
    if (tid == 0) {
        unsigned run = 0;
        s_start[0] = 0;
        for (int k = 1; k <= 256; ++k) {
            run += s_start[k];
            s_start[k] = run;
        }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) dest[r] = digit[r] >= 0 ? s_start[digit[r]] + s_cnt[wave][digit[r]] + local[r] : 0u;
    __syncthreads();                          // s_cnt and s_start are rewritten by the next step
}

// one workgroup a pair of sets
__global__ __launch_bounds__(kL2SortThreads) void l2_keep_kernel(const int* __restrict__ n1, int M1, const int* __restrict__ n2, int M2,
                                                                const unsigned long long* __restrict__ best12,
                                                                const unsigned long long* __restrict__ best21, const int* __restrict__ second,
                                                                int cross_check, double ratio, int max_distance2, int mm,
                                                                int* __restrict__ pairs, int* __restrict__ dist2, int* __restrict__ second2,
                                                                int* __restrict__ count) {
    __shared__ unsigned s_cnt[16][256];
    __shared__ unsigned s_start[257];
    __shared__ int s_d[kSiftMaxM];
    __shared__ unsigned short s_idx[2][kSiftMaxM];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long b = blockIdx.x;
    const int nq = min(max(n1[b], 0), M1), nt = min(max(n2[b], 0), M2);
    const unsigned long long* b12 = best12 + b * M1;
    const unsigned long long* b21 = best21 + b * M2;
    const int* sec = second + b * M1;
    int digit[4];
    unsigned dest[4];
    // the kept queries, in query order
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = 256 * wave + 64 * r + lane;
        bool kept = i < nq && nt >= 1;
        int d = 0;
        if (kept) {
            const unsigned long long key = b12[i];
            const int j = (int)(key & 4095u);
            d = (int)(key >> 12);
            if (cross_check) kept = (int)(b21[j] & 4095u) == i;
            if (ratio >= 0.0) kept = kept && nt >= 2 && (double)d < (ratio * ratio) * (double)sec[i];
            if (max_distance2 >= 0) kept = kept && d <= max_distance2;
        }
        if (i < kSiftMaxM) s_d[i] = d;
        digit[r] = kept ? 0 : -1;
    }
    l2_scatter(digit, dest, s_cnt, s_start);
    const int n = (int)s_start[1];
#pragma unroll
    for (int r = 0; r < 4; ++r)
        if (digit[r] >= 0) s_idx[0][dest[r]] = (unsigned short)(256 * wave + 64 * r + lane);
    __syncthreads();
    int cur = 0;
    for (int pass = 0; pass < 3; ++pass) {
        unsigned short idx[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int p = 256 * wave + 64 * r + lane;
            idx[r] = p < n ? s_idx[cur][p] : (unsigned short)0;
            digit[r] = p < n ? (s_d[idx[r]] >> (8 * pass)) & 255 : -1;
        }
        l2_scatter(digit, dest, s_cnt, s_start);
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (digit[r] >= 0) s_idx[cur ^ 1][dest[r]] = idx[r];
        __syncthreads();
        cur ^= 1;
    }
    const int written = min(n, mm);
    if (tid == 0) count[b] = written;
    int* op = pairs + b * mm * 2;
    for (int r = tid; r < mm; r += kL2SortThreads) {
        int i = -1, j = -1, d = -1, s2 = -1;
        if (r < written) {
            i = s_idx[cur][r];
            j = (int)(b12[i] & 4095u);
            d = s_d[i];
            s2 = sec[i];
        }
        op[2 * r] = i;
        op[2 * r + 1] = j;
        dist2[b * mm + r] = d;
        second2[b * mm + r] = s2;
    }
}

// the octaves of an H x W frame; false when the sizes are refused
static bool sift_pyramid(int64_t N, int32_t H, int32_t W, int32_t octaves, int32_t M, SiftPyr& py) {
    if (!(N >= 1 && N <= 65535 && H >= 1 && W >= 1 && H <= SKIMI_LENS_MAX_SIDE && W <= SKIMI_LENS_MAX_SIDE &&
          (int64_t)H * W <= SKIMI_CHESS_MAX_PIXELS && octaves >= 0 && octaves <= SKIMI_SIFT_MAX_OCTAVES && M >= 1 && M <= SKIMI_SIFT_MAX_FEATURES))
        return false;
    py = SiftPyr{};
    py.O = octaves;
    py.M = M;
    long P = 0, C = 0, G = 0;
    int w = W, h = H;
    for (int o = 0; o < octaves && std::min(w, h) >= SKIMI_SIFT_MIN_SIDE; ++o) {
        py.W[o] = w, py.H[o] = h;
        py.cap[o] = (int)std::min((long)w * h, (long)SKIMI_SIFT_MAX_CANDIDATES);
        py.poff[o] = P;
        P += (long)align_up((size_t)kSiftLayers * w * h, 4);
        for (int k = 0; k < kSiftS; ++k) {
            py.coff[kSiftS * o + k] = C, py.goff[kSiftS * o + k] = G;
            C += py.cap[o];
            G += (long)cdiv((int64_t)w * h, kSiftTile);
        }
        py.Oe = o + 1;
        w = (w + 1) / 2, h = (h + 1) / 2;
    }
    py.P = P, py.C = C, py.G = G;
    return true;
}

static size_t sift_ws_layout(int64_t N, const SiftPyr& py, void* ws, SiftWs* out) {
    unsigned char* p = static_cast<unsigned char*>(ws);
    const size_t nc = (size_t)N * py.C;
    const size_t o_key = 0, o_rxy = o_key + nc * 8, o_rsr = o_rxy + nc * 16, o_rpos = o_rsr + nc * 16, o_cand = o_rpos + nc * 16,
                 o_bc = o_cand + align_up(nc * 4, 16), o_seg = o_bc + align_up((size_t)N * py.G * 4, 16),
                 o_gauss = o_seg + align_up((size_t)N * kSiftSegs * 4, 16), end = o_gauss + (size_t)N * py.P * 4;
    if (out) {
        out->key = reinterpret_cast<unsigned long long*>(p + o_key);
        out->rxy = reinterpret_cast<double*>(p + o_rxy);
        out->rsr = reinterpret_cast<double*>(p + o_rsr);
        out->rpos = reinterpret_cast<int*>(p + o_rpos);
        out->cand = reinterpret_cast<int*>(p + o_cand);
        out->block_count = reinterpret_cast<unsigned*>(p + o_bc);
        out->seg_count = reinterpret_cast<int*>(p + o_seg);
        out->gauss = reinterpret_cast<float*>(p + o_gauss);
    }
    return end;
}

template <int SRC>
static void sift_blur(hipStream_t st, const void* src, long sstride, float* dst, long dstride, int W, int H, int64_t N, const float* taps,
                      int layer) {
    constexpr int radii[kSiftLayers] = SKIMI_SIFT_RADII;
    hipLaunchKernelGGL(sift_blur_kernel<SRC>, dim3((unsigned)(cdiv(W, kBlurTW) * cdiv(H, kBlurTH)), (unsigned)N), dim3(kSiftThreads), 0, st, src,
                       sstride, dst, dstride, W, H, taps + layer * kSiftTaps, radii[layer]);
}

}  // namespace skimi

using namespace skimi;

extern "C" {

size_t skimi_sift_workspace_bytes(int64_t N, int32_t H, int32_t W, int32_t octaves) {
    SiftPyr py;
    if (!sift_pyramid(N, H, W, octaves, 1, py)) return 0;
    return sift_ws_layout(N, py, nullptr, nullptr);
}

int skimi_sift_features(const uint8_t* frames, int64_t N, int32_t H, int32_t W, int32_t ch, int32_t octaves, int32_t max_features,
                        const double* roi, const float* taps, double* xy, int32_t* xy_level, int32_t* octave, int32_t* layer, double* sigma,
                        double* response, double* angle, uint8_t* desc, int32_t* count, int32_t* octave_count, void* ws, size_t ws_bytes,
                        void* stream) {
    SKIMI_CHECK_ARG(frames && taps && xy && xy_level && octave && layer && sigma && response && angle && desc && count && ws &&
                        (octave_count || octaves <= 0),
                    "skimi_sift_features: null pointer");
    SiftPyr py;
    SKIMI_CHECK_ARG(sift_pyramid(N, H, W, octaves, max_features, py),
                    "skimi_sift_features: need 1 <= N <= 65535 frames with sides in 1 .. %d and at most %d pixels, 0 .. %d octaves and 1 .. %d "
                    "features (N = %lld, H = %d, W = %d, octaves = %d, max_features = %d)",
                    SKIMI_LENS_MAX_SIDE, SKIMI_CHESS_MAX_PIXELS, SKIMI_SIFT_MAX_OCTAVES, SKIMI_SIFT_MAX_FEATURES, (long long)N, H, W, octaves,
                    max_features);
    SKIMI_CHECK_ARG(ch == 1 || ch == 3 || ch == 4, "skimi_sift_features: 1, 3 or 4 channels, got %d", ch);
    SKIMI_CHECK_ARG(ws_bytes >= skimi_sift_workspace_bytes(N, H, W, octaves), "skimi_sift_features: workspace too small (%zu < %zu bytes)",
                    ws_bytes, skimi_sift_workspace_bytes(N, H, W, octaves));
    SKIMI_CHECK_ARG(((uintptr_t)ws & 15) == 0 && ((uintptr_t)desc & 15) == 0,
                    "skimi_sift_features: the workspace and the descriptors must be 16-byte aligned");
    SiftWs w;
    sift_ws_layout(N, py, ws, &w);
    hipStream_t st = (hipStream_t)stream;
    const dim3 block(kSiftThreads);
    for (int o = 0; o < py.Oe; ++o) {
        const int Wo = py.W[o], Ho = py.H[o];
        const long plane = (long)Wo * Ho;
        float* G = w.gauss + py.poff[o];
        if (o == 0) {
            if (ch == 1)
                sift_blur<1>(st, frames, 0, G, py.P, Wo, Ho, N, taps, 0);
            else if (ch == 3)
                sift_blur<3>(st, frames, 0, G, py.P, Wo, Ho, N, taps, 0);
            else
                sift_blur<4>(st, frames, 0, G, py.P, Wo, Ho, N, taps, 0);
        } else {
            hipLaunchKernelGGL(sift_half_kernel, dim3((unsigned)cdiv(plane, kSiftThreads), (unsigned)N), block, 0, st,
                               (const float*)(w.gauss + py.poff[o - 1] + (long)kSiftS * py.W[o - 1] * py.H[o - 1]), G, py.P, py.W[o - 1], Wo, Ho);
        }
        for (int i = 1; i < kSiftLayers; ++i) sift_blur<0>(st, G + (i - 1) * plane, py.P, G + i * plane, py.P, Wo, Ho, N, taps, i);
    }
    if (py.Oe > 0) {
        const dim3 groups((unsigned)cdiv((long)W * H, kSiftTile), (unsigned)(kSiftS * py.Oe), (unsigned)N);
        hipLaunchKernelGGL(sift_count_kernel, groups, block, 0, st, py, (const float*)w.gauss, w.block_count);
        hipLaunchKernelGGL(sift_write_kernel, groups, block, 0, st, py, (const float*)w.gauss, (const unsigned*)w.block_count, w.cand,
                           w.seg_count);
        hipLaunchKernelGGL(sift_refine_kernel, dim3((unsigned)cdiv(py.cap[0], kSiftThreads), (unsigned)(kSiftS * py.Oe), (unsigned)N), block, 0,
                           st, py, (const float*)w.gauss, (const int*)w.cand, (const int*)w.seg_count, roi, w.key, w.rxy, w.rsr, w.rpos);
    }
    hipLaunchKernelGGL(sift_select_kernel, dim3((unsigned)N), block, 0, st, py, (const int*)w.seg_count, (const unsigned long long*)w.key,
                       (const double*)w.rxy, (const double*)w.rsr, (const int*)w.rpos, xy, xy_level, octave, layer, sigma, response, angle, desc,
                       count, octave_count);
    if (py.Oe > 0) {
        const long total = (long)N * py.M;
        hipLaunchKernelGGL(sift_describe_kernel, dim3((unsigned)cdiv(total, kSiftWaves)), block, 0, st, py, (const float*)w.gauss,
                           (const int*)xy_level, (const int*)octave, (const int*)layer, (const double*)sigma, (const int*)count, total, angle,
                           desc);
    }
    SKIMI_LAUNCH_CHECK();
    return SKIMI_OK;
}

int skimi_match_l2(const uint8_t* d1, const int32_t* n1, int32_t M1, const uint8_t* d2, const int32_t* n2, int32_t M2, int64_t B,
                   int32_t cross_check, double ratio, int32_t max_distance2, int32_t max_matches, int32_t* pairs, int32_t* dist2,
                   int32_t* second2, int32_t* count, void* ws, size_t ws_bytes, void* stream) {
    SKIMI_CHECK_ARG(d1 && n1 && d2 && n2 && pairs && dist2 && second2 && count && ws, "skimi_match_l2: null pointer");
    SKIMI_CHECK_ARG(B >= 1 && B <= 65535, "skimi_match_l2: need 1 <= B <= 65535 pairs of sets, got %lld", (long long)B);
    SKIMI_CHECK_ARG(M1 >= 1 && M1 <= SKIMI_SIFT_MAX_FEATURES && M2 >= 1 && M2 <= SKIMI_SIFT_MAX_FEATURES,
                    "skimi_match_l2: the sets hold 1 .. %d descriptors, got %d and %d", SKIMI_SIFT_MAX_FEATURES, M1, M2);
    SKIMI_CHECK_ARG(max_matches >= 1 && max_matches <= SKIMI_SIFT_MAX_FEATURES, "skimi_match_l2: max_matches must be in 1 .. %d, got %d",
                    SKIMI_SIFT_MAX_FEATURES, max_matches);
    SKIMI_CHECK_ARG(ratio == ratio, "skimi_match_l2: ratio must not be NaN (negative: no ratio test)");
    const size_t need = (size_t)B * ((size_t)M1 + M2) * 8 + (size_t)B * M1 * 4;
    SKIMI_CHECK_ARG(ws_bytes >= need, "skimi_match_l2: workspace too small (%zu < %zu bytes)", ws_bytes, need);
    SKIMI_CHECK_ARG(((uintptr_t)d1 & 15) == 0 && ((uintptr_t)d2 & 15) == 0 && ((uintptr_t)ws & 15) == 0,
                    "skimi_match_l2: descriptors and workspace must be 16-byte aligned");
    unsigned long long* best12 = static_cast<unsigned long long*>(ws);
    unsigned long long* best21 = best12 + (size_t)B * M1;
    int* second = reinterpret_cast<int*>(best21 + (size_t)B * M2);
    hipStream_t st = (hipStream_t)stream;
    const int mq = cross_check ? std::max(M1, M2) : M1;
    hipLaunchKernelGGL(l2_nn_kernel, dim3((unsigned)cdiv(mq, kL2Q), (unsigned)B, cross_check ? 2u : 1u), dim3(kSiftThreads), 0, st, d1,
                       (const int*)n1, M1, d2, (const int*)n2, M2, best12, best21, second);
    hipLaunchKernelGGL(l2_keep_kernel, dim3((unsigned)B), dim3(kL2SortThreads), 0, st, (const int*)n1, M1, (const int*)n2, M2,
                       (const unsigned long long*)best12, (const unsigned long long*)best21, (const int*)second, cross_check, ratio,
                       max_distance2, max_matches, pairs, dist2, second2, count);
    SKIMI_LAUNCH_CHECK();
    return SKIMI_OK;
}

}  // extern "C"
