// ORB-style image features on whole frames and a brute-force Hamming matcher (camera_position.py:181-226,
// estimate_camera_pose_from_ORB = cv2.ORB_create + cv2.BFMatcher) under the project's own rules: DESIGN §2 "Image features", the
// block in include/skimi.h; tests/features_restated.py evaluates the same expressions.
//   gray, shrink, blur   the pyramid of a frame: bytes in the workspace, level after level
//   fast                 the segment-test score of every level in one launch: a tile with its radius-3 halo in LDS
//   count / write        compact.h's exact compaction in pixel order: 3 x 3 non-maximum suppression and the box
//   harris               the Harris response of every candidate, a candidate a lane
//   select               one workgroup a (frame, level): compact.h's exact radix selection of the q_l largest responses
//                        (ties to the smaller pixel), written in pixel order behind the levels before it
//   describe             one wave a keypoint: the two moments by reduce.h's wave_sum, the direction as an integer argmax, the
//                        256 bits as four 64-lane ballots
//   match                one workgroup a pair of sets: train descriptors staged in LDS, a query a lane, the minimum of a packed
//                        (distance << 16 | index) key; cross check, ratio, a stable counting sort over the 257 distances
// Every stage is integer: the results are bitwise reproducible and a frame's do not depend on the batch around it.
#include "common.h"
#include "compact.h"
#include "gray.h"
#include "reduce.h"

namespace skimi {

constexpr int kOrbThreads = 256;
constexpr int kOrbWaves = kOrbThreads / 64;
constexpr int kFastTW = 64, kFastTH = 16, kFastHalo = 3;
constexpr int kFastLW = kFastTW + 2 * kFastHalo, kFastLH = kFastTH + 2 * kFastHalo;   // 70 x 22
constexpr int kFastLS = 72;                                                           // bytes of a tile row in LDS
constexpr long kOrbTile = 4096;               // pixels of a workgroup of the candidate launches
constexpr int kMatchStage = 512;              // train descriptors staged at a time (16 KiB)
constexpr int kMatchThreads = 1024;           // one workgroup a pair of sets: sixteen waves share the staged descriptors
constexpr int kOrbMaxM = SKIMI_ORB_MAX_FEATURES;

__constant__ int kOrbCos[32] = SKIMI_ORB_COS;
__constant__ int kOrbSin[32] = SKIMI_ORB_SIN;

// the levels of one frame's pyramid and where each starts in the per-frame arrays of the workspace
struct OrbPyr {
    int L, M, threshold;
    int W[SKIMI_ORB_MAX_LEVELS], H[SKIMI_ORB_MAX_LEVELS], q[SKIMI_ORB_MAX_LEVELS], cap[SKIMI_ORB_MAX_LEVELS];
    long poff[SKIMI_ORB_MAX_LEVELS], coff[SKIMI_ORB_MAX_LEVELS], goff[SKIMI_ORB_MAX_LEVELS];
    long P, C, G;                             // pixels, candidate rows and candidate workgroups of a frame
};

struct OrbWs {
    long long* harris;                        // [N, C]
    int* cand;                                // [N, C] pixel index in its level
    unsigned* block_count;                    // [N, G]
    unsigned char *gray, *blur, *score;       // [N, P] each
};

// ---- the pyramid ----
template <int CH>
__global__ __launch_bounds__(kOrbThreads) void orb_gray_kernel(const unsigned char* __restrict__ frames, long n, long P,
                                                               unsigned char* __restrict__ gray) {
    const long f = blockIdx.y, i = (long)blockIdx.x * kOrbThreads + threadIdx.x;
    if (i < n) gray[f * P + i] = (unsigned char)orb_gray<CH>(frames + (f * n + i) * CH);
}

__device__ __forceinline__ void orb_axis(int x, int ns, int nd, int& x0, int& x1, int& a) {
    const long n = (2L * x + 1) * ns - nd, den = 2L * nd;   // n >= 0: ns >= nd
    const long q = n / den;
    a = (int)(((n - q * den) * 256) / den);
    x0 = min((int)q, ns - 1);
    x1 = min((int)q + 1, ns - 1);
}

__global__ __launch_bounds__(kOrbThreads) void orb_shrink_kernel(unsigned char* __restrict__ gray, long P, long soff, int Ws, int Hs,
                                                                 long doff, int Wd, int Hd) {
    const long f = blockIdx.y, i = (long)blockIdx.x * kOrbThreads + threadIdx.x;
    if (i >= (long)Wd * Hd) return;
    const int y = (int)(i / Wd), x = (int)(i - (long)y * Wd);
    int x0, x1, ax, y0, y1, ay;
    orb_axis(x, Ws, Wd, x0, x1, ax);
    orb_axis(y, Hs, Hd, y0, y1, ay);
    const unsigned char* s = gray + f * P + soff;
    const int p00 = s[(long)y0 * Ws + x0], p01 = s[(long)y0 * Ws + x1], p10 = s[(long)y1 * Ws + x0], p11 = s[(long)y1 * Ws + x1];
    const int v = (256 - ay) * ((256 - ax) * p00 + ax * p01) + ay * ((256 - ax) * p10 + ax * p11);
    gray[f * P + doff + i] = (unsigned char)((v + (1 << 15)) >> 16);
}

// grid (groups of level 0, L, frames)
__global__ __launch_bounds__(kOrbThreads) void orb_blur_kernel(OrbPyr py, const unsigned char* __restrict__ gray,
                                                               unsigned char* __restrict__ blur) {
    const int l = blockIdx.y, W = py.W[l], H = py.H[l];
    const long f = blockIdx.z, i = (long)blockIdx.x * kOrbThreads + threadIdx.x;
    if (i >= (long)W * H) return;
    const int y = (int)(i / W), x = (int)(i - (long)y * W);
    const unsigned char* g = gray + f * py.P + py.poff[l];
    constexpr int k[5] = {1, 4, 6, 4, 1};
    int v = 0;
#pragma unroll
    for (int dy = 0; dy < 5; ++dy) {
        const unsigned char* row = g + (long)min(max(y + dy - 2, 0), H - 1) * W;
        int r = 0;
#pragma unroll
        for (int dx = 0; dx < 5; ++dx) r += k[dx] * (int)row[min(max(x + dx - 2, 0), W - 1)];
        v += k[dy] * r;
    }
    blur[f * py.P + py.poff[l] + i] = (unsigned char)((v + 128) >> 8);
}

// ---- the segment-test score: grid (tiles of level 0, L, frames); a 64 x 16 tile and its halo in LDS ----
// The stored map holds s where s > threshold and 0 elsewhere: the suppression compares corners only against larger values.
__global__ __launch_bounds__(kOrbThreads) void orb_fast_kernel(OrbPyr py, const unsigned char* __restrict__ gray,
                                                               unsigned char* __restrict__ score) {
    __shared__ unsigned char s_t[kFastLH][kFastLS];
    const int l = blockIdx.y, W = py.W[l], H = py.H[l];
    const int tilesx = (W + kFastTW - 1) / kFastTW, tilesy = (H + kFastTH - 1) / kFastTH;
    if ((int)blockIdx.x >= tilesx * tilesy) return;
    const int tid = threadIdx.x, tx = tid & 63, ty = tid >> 6;
    const int bx = ((int)blockIdx.x % tilesx) * kFastTW, by = ((int)blockIdx.x / tilesx) * kFastTH;
    const long f = blockIdx.z, base = f * py.P + py.poff[l];
    const unsigned char* g = gray + base;
    unsigned char* out = score + base;
    constexpr int B = SKIMI_ORB_BORDER;
    // a tile without a pixel of the candidate region (the same for every thread)
    const bool any = bx < W - B && bx + kFastTW > B && by < H - B && by + kFastTH > B;
    if (any) {
        for (int idx = tid; idx < kFastLH * kFastLW; idx += kOrbThreads) {
            const int r = idx / kFastLW, c = idx - r * kFastLW;
            const int gx = min(max(bx - kFastHalo + c, 0), W - 1), gy = min(max(by - kFastHalo + r, 0), H - 1);
            s_t[r][c] = g[(long)gy * W + gx];
        }
    }
    __syncthreads();
    constexpr int ox[16] = {0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1};
    constexpr int oy[16] = {-3, -3, -2, -1, 0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3};
    const int thr = py.threshold;
    const int px = bx + tx;
#pragma unroll
    for (int k = 0; k < kFastTH / kOrbWaves; ++k) {
        const int row = ty + k * kOrbWaves, pyx = by + row;
        if (px >= W || pyx >= H) continue;
        int s = 0;
        if (any && px >= B && px < W - B && pyx >= B && pyx < H - B) {
            const int lc = tx + kFastHalo, lr = row + kFastHalo;
            const int p = s_t[lr][lc];
            // nine contiguous ring pixels hold two neighbouring compass pixels: without two on one side there is no corner
            const int c0 = (int)s_t[lr - 3][lc] - p, c4 = (int)s_t[lr][lc + 3] - p, c8 = (int)s_t[lr + 3][lc] - p,
                      c12 = (int)s_t[lr][lc - 3] - p;
            const int hi = (c0 > thr) + (c4 > thr) + (c8 > thr) + (c12 > thr);
            const int lo = (c0 < -thr) + (c4 < -thr) + (c8 < -thr) + (c12 < -thr);
            if (hi >= 2 || lo >= 2) {
                int d[16];
#pragma unroll
                for (int n = 0; n < 16; ++n) d[n] = (int)s_t[lr + oy[n]][lc + ox[n]] - p;
                // the minimum and the maximum of the nine from n on, by doubling: 2, 4, 8, then the ninth
                int mn2[16], mx2[16], mn4[16], mx4[16];
#pragma unroll
                for (int n = 0; n < 16; ++n) {
                    mn2[n] = min(d[n], d[(n + 1) & 15]);
                    mx2[n] = max(d[n], d[(n + 1) & 15]);
                }
#pragma unroll
                for (int n = 0; n < 16; ++n) {
                    mn4[n] = min(mn2[n], mn2[(n + 2) & 15]);
                    mx4[n] = max(mx2[n], mx2[(n + 2) & 15]);
                }
                int best = -256;
#pragma unroll
                for (int n = 0; n < 16; ++n) {
                    const int mn9 = min(min(mn4[n], mn4[(n + 4) & 15]), d[(n + 8) & 15]);
                    const int mx9 = max(max(mx4[n], mx4[(n + 4) & 15]), d[(n + 8) & 15]);
                    best = max(best, max(mn9, -mx9));
                }
                s = best > thr ? best : 0;
            }
        }
        out[(long)pyx * W + px] = (unsigned char)s;
    }
}

// rules 3: a corner that is the maximum of its 3 x 3 window (ties to the earlier pixel) and lies in the frame's box
__device__ __forceinline__ void orb_level0_xy(int x, int y, int W0, int H0, int W, int H, double& X, double& Y) {
    X = (((double)x + 0.5) * (double)W0) / (double)W - 0.5;
    Y = (((double)y + 0.5) * (double)H0) / (double)H - 0.5;
}

__device__ inline bool orb_candidate(const unsigned char* __restrict__ S, int W, int H, int W0, int H0, int i, int thr,
                                     const double* __restrict__ box) {
    const int v = S[i];
    if (v <= thr) return false;               // also: v > 0 only inside the border, so the window is inside the level
    const int y = i / W, x = i - y * W;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            if (dx == 0 && dy == 0) continue;
            const int q = S[i + dy * W + dx];
            if ((dy < 0 || (dy == 0 && dx < 0)) ? !(v > q) : !(v >= q)) return false;
        }
    if (box) {
        double X, Y;
        orb_level0_xy(x, y, W0, H0, W, H, X, Y);
        if (!(X >= box[0] && X < box[2] && Y >= box[1] && Y < box[3])) return false;
    }
    return true;
}

// rule 4 at a candidate (at least SKIMI_ORB_BORDER from every edge)
__device__ inline long long orb_harris(const unsigned char* __restrict__ g, int W, int x, int y) {
    long long a = 0, b = 0, c = 0;
    for (int dy = -3; dy <= 3; ++dy) {
        const unsigned char* r0 = g + (long)(y + dy - 1) * W + x;
        const unsigned char *r1 = r0 + W, *r2 = r1 + W;
#pragma unroll
        for (int dx = -3; dx <= 3; ++dx) {
            const int p00 = r0[dx - 1], p01 = r0[dx], p02 = r0[dx + 1], p10 = r1[dx - 1], p12 = r1[dx + 1], p20 = r2[dx - 1],
                      p21 = r2[dx], p22 = r2[dx + 1];
            const int ix = (p02 + 2 * p12 + p22) - (p00 + 2 * p10 + p20), iy = (p20 + 2 * p21 + p22) - (p00 + 2 * p01 + p02);
            a += ix * ix;
            b += iy * iy;
            c += ix * iy;
        }
    }
    return 25 * (a * b - c * c) - (a + b) * (a + b);
}

// ---- candidates per workgroup of kOrbTile consecutive pixels; grid (groups of level 0, L, frames) ----
__global__ __launch_bounds__(kOrbThreads) void orb_count_kernel(OrbPyr py, const unsigned char* __restrict__ score,
                                                                const double* __restrict__ roi, unsigned* __restrict__ block_count) {
    __shared__ unsigned s_cnt;
    const int l = blockIdx.y, W = py.W[l], H = py.H[l];
    const long n = (long)W * H, g = blockIdx.x, f = blockIdx.z;
    if (g * kOrbTile >= n) return;
    const unsigned char* S = score + f * py.P + py.poff[l];
    const double* box = roi ? roi + 4 * f : nullptr;
    const long beg = g * kOrbTile, end = min(beg + kOrbTile, n);
    const unsigned cnt = tile_count<kOrbThreads>(
        beg, end, s_cnt, [&](long i) { return orb_candidate(S, W, H, py.W[0], py.H[0], (int)i, py.threshold, box); });
    if (threadIdx.x == 0) block_count[f * py.G + py.goff[l] + g] = cnt;
}

__global__ __launch_bounds__(kOrbThreads) void orb_write_kernel(OrbPyr py, const unsigned char* __restrict__ score,
                                                                const double* __restrict__ roi, const unsigned* __restrict__ block_count,
                                                                int* __restrict__ cand, int* __restrict__ level_count) {
    __shared__ unsigned s_total, s_offset;
    __shared__ unsigned s_wtot[2][kOrbWaves];
    const int l = blockIdx.y, W = py.W[l], H = py.H[l];
    const long n = (long)W * H, g = blockIdx.x, f = blockIdx.z;
    if (g * kOrbTile >= n) return;
    const int groups = (int)((n + kOrbTile - 1) / kOrbTile);
    const unsigned char* S = score + f * py.P + py.poff[l];
    const double* box = roi ? roi + 4 * f : nullptr;
    const unsigned* bc = block_count + f * py.G + py.goff[l];
    group_offsets<kOrbThreads>(bc, groups, g, s_total, s_offset);
    if (g == 0 && threadIdx.x == 0) level_count[f * py.L + l] = (int)s_total;
    if (bc[g] == 0) return;                   // uniform
    int* oc = cand + f * py.C + py.coff[l];
    const long cap = py.cap[l];
    const long beg = g * kOrbTile, end = min(beg + kOrbTile, n);
    ordered_write<kOrbThreads>(
        beg, end, (long)s_offset, s_wtot, [&](long i) { return orb_candidate(S, W, H, py.W[0], py.H[0], (int)i, py.threshold, box); },
        [&](long i, long row) {
            if (row < cap) oc[row] = (int)i;
        });
}

// ---- the response of every candidate: grid (rows of level 0's capacity / threads, L, frames) ----
__global__ __launch_bounds__(kOrbThreads) void orb_harris_kernel(OrbPyr py, const unsigned char* __restrict__ gray, const int* __restrict__ cand,
                                                                 const int* __restrict__ level_count, long long* __restrict__ harris) {
    const int l = blockIdx.y, W = py.W[l];
    const long f = blockIdx.z, r = (long)blockIdx.x * kOrbThreads + threadIdx.x;
    if (r >= min(level_count[f * py.L + l], py.cap[l])) return;
    const int p = cand[f * py.C + py.coff[l] + r], y = p / W, x = p - y * W;
    harris[f * py.C + py.coff[l] + r] = orb_harris(gray + f * py.P + py.poff[l], W, x, y);
}

// ---- selection: grid (L, frames) ----
__device__ __forceinline__ unsigned long long orb_key(long long h) { return (unsigned long long)h ^ (1ull << 63); }

__global__ __launch_bounds__(kOrbThreads) void orb_select_kernel(OrbPyr py, const unsigned char* __restrict__ score,
                                                                 const int* __restrict__ cand, const long long* __restrict__ harris,
                                                                 const int* __restrict__ level_count, int* __restrict__ xy_level,
                                                                 double* __restrict__ xy, int* __restrict__ level, int* __restrict__ direction,
                                                                 int* __restrict__ oscore, long long* __restrict__ oharris, int* __restrict__ desc,
                                                                 int* __restrict__ count) {
    __shared__ unsigned s_hist[256];
    __shared__ unsigned s_digit, s_need;
    __shared__ unsigned s_wtot[2][2][kOrbWaves];
    const int l = blockIdx.x, W = py.W[l], H = py.H[l], M = py.M, tid = threadIdx.x;
    const long f = blockIdx.y;
    const int* lc = level_count + f * py.L;
    int base = 0, total = 0;
    for (int k = 0; k < py.L; ++k) {
        const int kept = min(min(lc[k], py.cap[k]), py.q[k]);
        if (k < l) base += kept;
        total += kept;
    }
    if (l == 0) {                             // the frame's count and the rows behind it
        if (tid == 0) count[f] = total;
        for (long r = (long)total + tid; r < M; r += kOrbThreads) {
            const long o = f * M + r;
            xy_level[2 * o] = xy_level[2 * o + 1] = -1;
            xy[2 * o] = xy[2 * o + 1] = -1.0;
            level[o] = direction[o] = -1;
            oscore[o] = 0;
            oharris[o] = 0;
#pragma unroll
            for (int w = 0; w < 8; ++w) desc[8 * o + w] = 0;
        }
    }
    const int n = min(lc[l], py.cap[l]), q = py.q[l];
    if (n == 0 || q == 0) return;
    const int* ci = cand + f * py.C + py.coff[l];
    const long long* ch = harris + f * py.C + py.coff[l];
    // the key T of descending rank q - 1 and how many of the keys equal to it are kept; n <= q keeps everything
    unsigned long long T = 0;
    unsigned need = (unsigned)q;
    if (n > q)
        select_threshold<kOrbThreads>(
            (unsigned)q,
            [&](auto&& add) {
                for (int i = tid; i < n; i += kOrbThreads) add(orb_key(ch[i]));
            },
            s_hist, s_digit, s_need, T, need);
    const unsigned char* S = score + f * py.P + py.poff[l];
    long row0 = base;
    unsigned eq0 = 0;
    int buf = 0;
    for (int i0 = 0; i0 < n; i0 += kOrbThreads) {        // uniform trip count
        const int i = i0 + tid;
        const bool live = i < n;
        const unsigned long long key = live ? orb_key(ch[i]) : 0;
        unsigned rank, chunk;
        if (select_rank<kOrbWaves>(key, live, n > q, T, need, eq0, s_wtot[buf], rank, chunk)) {
            const long r = row0 + rank;
            if (r < M) {
                const long o = f * M + r;
                const int p = ci[i], y = p / W, x = p - y * W;
                double X, Y;
                orb_level0_xy(x, y, py.W[0], py.H[0], W, H, X, Y);
                xy_level[2 * o] = x;
                xy_level[2 * o + 1] = y;
                xy[2 * o] = X;
                xy[2 * o + 1] = Y;
                level[o] = l;
                oscore[o] = S[p];
                oharris[o] = ch[i];
            }
        }
        row0 += chunk;
        buf ^= 1;
    }
}

// ---- orientation and descriptor: one wave a row ----
__global__ __launch_bounds__(kOrbThreads) void orb_describe_kernel(OrbPyr py, const unsigned char* __restrict__ gray,
                                                                   const unsigned char* __restrict__ blur, const signed char* __restrict__ pattern,
                                                                   const int* __restrict__ xy_level, const int* __restrict__ level,
                                                                   const int* __restrict__ count, long total, int* __restrict__ direction,
                                                                   int* __restrict__ desc) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long o = (long)blockIdx.x * kOrbWaves + wave;
    if (o >= total) return;
    const long f = o / py.M;
    if ((int)(o - f * py.M) >= count[f]) return;
    const int l = level[o], W = py.W[l], x = xy_level[2 * o], y = xy_level[2 * o + 1];
    const unsigned char* g = gray + f * py.P + py.poff[l] + (long)y * W + x;
    const unsigned char* b = blur + f * py.P + py.poff[l] + (long)y * W + x;
    int m10 = 0, m01 = 0;
    for (int k = lane; k < 31 * 31; k += 64) {
        const int v = k / 31 - 15, u = k - (v + 15) * 31 - 15;
        if (u * u + v * v <= 225) {
            const int I = g[v * W + u];
            m10 += u * I;
            m01 += v * I;
        }
    }
    m10 = wave_sum(m10);
    m01 = wave_sum(m01);
    int dir = 0;
    long long top = (long long)m10 * kOrbCos[0] + (long long)m01 * kOrbSin[0];
    for (int k = 1; k < 32; ++k) {
        const long long v = (long long)m10 * kOrbCos[k] + (long long)m01 * kOrbSin[k];
        if (v > top) {
            top = v;
            dir = k;
        }
    }
    const int* pat = reinterpret_cast<const int*>(pattern) + dir * 256;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int w = pat[c * 64 + lane];
        const int ax = (signed char)(w & 255), ay = (signed char)((w >> 8) & 255), bx = (signed char)((w >> 16) & 255),
                  by = (signed char)((w >> 24) & 255);
        const unsigned long long m = __ballot(b[ay * W + ax] < b[by * W + bx]);
        if (lane == 0) {
            desc[8 * o + 2 * c] = (int)(unsigned)(m & 0xFFFFFFFFull);
            desc[8 * o + 2 * c + 1] = (int)(unsigned)(m >> 32);
        }
    }
    if (lane == 0) direction[o] = dir;
}

// ---- the matcher: one workgroup a pair of sets ----
// best and second-best key (distance << 16 | train index) of every query of `dq` against the `nt` descriptors of `dt`
__device__ inline void match_pass(const unsigned* __restrict__ dq, int nq, const unsigned* __restrict__ dt, int nt, unsigned (*s_stage)[8],
                                  unsigned* s_best, unsigned short* s_second) {
    const int tid = threadIdx.x;
    for (int i0 = 0; i0 < nq; i0 += kMatchThreads) {       // uniform trip counts: the barriers are met by every thread
        const int i = i0 + tid;
        unsigned q[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (i < nq) {
#pragma unroll
            for (int w = 0; w < 8; ++w) q[w] = dq[8 * (long)i + w];
        }
        unsigned b1 = 0xFFFFFFFFu, b2 = 0xFFFFFFFFu;
        for (int t0 = 0; t0 < nt; t0 += kMatchStage) {
            const int cnt = min(kMatchStage, nt - t0);
            __syncthreads();
            for (int k = tid; k < cnt * 8; k += kMatchThreads) (&s_stage[0][0])[k] = dt[8 * (long)t0 + k];
            __syncthreads();
            if (i < nq) {
                for (int j = 0; j < cnt; ++j) {
                    const uint4 lo = *reinterpret_cast<const uint4*>(&s_stage[j][0]), hi = *reinterpret_cast<const uint4*>(&s_stage[j][4]);
                    const unsigned d = __popc(q[0] ^ lo.x) + __popc(q[1] ^ lo.y) + __popc(q[2] ^ lo.z) + __popc(q[3] ^ lo.w) +
                                       __popc(q[4] ^ hi.x) + __popc(q[5] ^ hi.y) + __popc(q[6] ^ hi.z) + __popc(q[7] ^ hi.w);
                    const unsigned key = (d << 16) | (unsigned)(t0 + j);
                    b2 = min(b2, max(b1, key));
                    b1 = min(b1, key);
                }
            }
        }
        if (i < nq) {
            s_best[i] = b1;
            if (s_second) s_second[i] = b2 == 0xFFFFFFFFu ? (unsigned short)0xFFFF : (unsigned short)(b2 >> 16);
        }
    }
    __syncthreads();
}

__global__ __launch_bounds__(kMatchThreads) void match_hamming_kernel(const unsigned* __restrict__ d1, const int* __restrict__ n1, int M1,
                                                                    const unsigned* __restrict__ d2, const int* __restrict__ n2, int M2,
                                                                    int cross_check, double ratio, int max_distance, int mm,
                                                                    int* __restrict__ pairs, int* __restrict__ dist, int* __restrict__ count) {
    __shared__ __attribute__((aligned(16))) unsigned s_stage[kMatchStage][8];
    __shared__ unsigned s_best12[kOrbMaxM], s_best21[kOrbMaxM];
    __shared__ unsigned short s_second[kOrbMaxM];        // the second distance, then the kept distance (0xFFFF: dropped)
    __shared__ unsigned s_start[257 + 1];
    __shared__ unsigned short s_chunk[kMatchThreads];
    const int tid = threadIdx.x;
    const long b = blockIdx.x;
    const int nq = min(max(n1[b], 0), M1), nt = min(max(n2[b], 0), M2);
    const unsigned* q = d1 + b * M1 * 8;
    const unsigned* t = d2 + b * M2 * 8;
    int* op = pairs + b * mm * 2;
    int* od = dist + b * mm;
    match_pass(q, nq, t, nt, s_stage, s_best12, s_second);
    if (cross_check) match_pass(t, nt, q, nq, s_stage, s_best21, nullptr);
    for (int k = tid; k < 258; k += kMatchThreads) s_start[k] = 0;
    __syncthreads();
    for (int i = tid; i < nq; i += kMatchThreads) {
        bool kept = nt >= 1;
        unsigned d = 0;
        if (kept) {
            const unsigned key = s_best12[i];
            const int j = (int)(key & 0xFFFFu);
            d = key >> 16;
            if (cross_check) kept = (int)(s_best21[j] & 0xFFFFu) == i;
            if (ratio >= 0.0) kept = kept && nt >= 2 && (double)d < ratio * (double)s_second[i];
            if (max_distance >= 0) kept = kept && (int)d <= max_distance;
        }
        s_second[i] = kept ? (unsigned short)d : (unsigned short)0xFFFF;
        if (kept) atomicAdd(&s_start[d + 1], 1u);        // the histogram, one bin up: the scan below leaves the bins' starts
    }
    __syncthreads();
    if (tid == 0) {
        unsigned run = 0;
        for (int k = 0; k <= 257; ++k) {
            run += s_start[k];
            s_start[k] = run;
        }
    }
    __syncthreads();
    const int total = (int)s_start[257], written = min(total, mm);
    if (tid == 0) count[b] = written;
    for (int r = written + tid; r < mm; r += kMatchThreads) {
        op[2 * r] = op[2 * r + 1] = -1;
        od[r] = -1;
    }
    for (int i0 = 0; i0 < nq; i0 += kMatchThreads) {       // uniform trip count
        const int i = i0 + tid;
        const unsigned short d = i < nq ? s_second[i] : (unsigned short)0xFFFF;
        s_chunk[tid] = d;
        __syncthreads();
        if (d != 0xFFFF) {
            unsigned rank = 0;
            for (int k = 0; k < tid; ++k) rank += s_chunk[k] == d;
            const unsigned row = s_start[d] + rank;
            if (row < (unsigned)mm) {
                op[2 * row] = i;
                op[2 * row + 1] = (int)(s_best12[i] & 0xFFFFu);
                od[row] = d;
            }
        }
        __syncthreads();
        if (d != 0xFFFF) atomicAdd(&s_start[d], 1u);
        __syncthreads();
    }
}

// the pyramid of an H x W frame; false when the sizes are refused
static bool orb_pyramid(int64_t N, int32_t H, int32_t W, int32_t levels, int32_t M, OrbPyr& py) {
    if (!(N >= 1 && N <= 65535 && H >= 1 && W >= 1 && H <= SKIMI_LENS_MAX_SIDE && W <= SKIMI_LENS_MAX_SIDE &&
          (int64_t)H * W <= SKIMI_CHESS_MAX_PIXELS && levels >= 1 && levels <= SKIMI_ORB_MAX_LEVELS && M >= 1 && M <= SKIMI_ORB_MAX_FEATURES))
        return false;
    py = OrbPyr{};
    py.L = levels;
    py.M = M;
    int64_t p5 = 1, p6 = 1, wsum = 0, w[SKIMI_ORB_MAX_LEVELS];
    long P = 0, C = 0, G = 0;
    for (int l = 0; l < levels; ++l) {
        py.W[l] = (int)((2 * (int64_t)W * p5 + p6) / (2 * p6));
        py.H[l] = (int)((2 * (int64_t)H * p5 + p6) / (2 * p6));
        if (py.W[l] < 1 || py.H[l] < 1) return false;
        py.cap[l] = ((py.W[l] + 1) / 2) * ((py.H[l] + 1) / 2);   // no two neighbours survive the suppression
        py.poff[l] = P, py.coff[l] = C, py.goff[l] = G;
        P += (long)align_up((size_t)py.W[l] * py.H[l], 16);
        C += py.cap[l];
        G += (long)cdiv((int64_t)py.W[l] * py.H[l], kOrbTile);
        p5 *= 5, p6 *= 6;
    }
    py.P = P, py.C = C, py.G = G;
    p5 = 1;
    for (int l = 0; l < levels; ++l) {
        p6 = 1;
        for (int k = 0; k < levels - 1 - l; ++k) p6 *= 6;
        w[l] = p5 * p6;
        wsum += w[l];
        p5 *= 5;
    }
    int rest = M;
    for (int l = 1; l < levels; ++l) {
        py.q[l] = (int)((int64_t)M * w[l] / wsum);
        rest -= py.q[l];
    }
    py.q[0] = rest;
    return true;
}

static size_t orb_ws_layout(int64_t N, const OrbPyr& py, void* ws, OrbWs* out) {
    size_t o = 0;
    unsigned char* p = static_cast<unsigned char*>(ws);
    const size_t nh = align_up((size_t)N * py.C * 8, 16), nc = align_up((size_t)N * py.C * 4, 16), nb = align_up((size_t)N * py.G * 4, 16),
                 np = (size_t)N * py.P;
    if (out) {
        out->harris = reinterpret_cast<long long*>(p + o);
        out->cand = reinterpret_cast<int*>(p + o + nh);
        out->block_count = reinterpret_cast<unsigned*>(p + o + nh + nc);
        out->gray = p + o + nh + nc + nb;
        out->blur = out->gray + np;
        out->score = out->blur + np;
    }
    return nh + nc + nb + 3 * np;
}

}  // namespace skimi

using namespace skimi;

extern "C" {

size_t skimi_orb_workspace_bytes(int64_t N, int32_t H, int32_t W, int32_t levels) {
    OrbPyr py;
    if (!orb_pyramid(N, H, W, levels, 1, py)) return 0;
    return orb_ws_layout(N, py, nullptr, nullptr);
}

int skimi_orb_features(const uint8_t* frames, int64_t N, int32_t H, int32_t W, int32_t ch, int32_t levels, int32_t threshold,
                       int32_t max_features, const double* roi, const int8_t* pattern, int32_t* xy_level, double* xy, int32_t* level,
                       int32_t* direction, int32_t* score, int64_t* harris, int32_t* desc, int32_t* count, int32_t* level_count, void* ws,
                       size_t ws_bytes, void* stream) {
    SKIMI_CHECK_ARG(frames && pattern && xy_level && xy && level && direction && score && harris && desc && count && level_count && ws,
                    "skimi_orb_features: null pointer");
    OrbPyr py;
    SKIMI_CHECK_ARG(orb_pyramid(N, H, W, levels, max_features, py),
                    "skimi_orb_features: need 1 <= N <= 65535 frames with sides in 1 .. %d and at most %d pixels, 1 .. %d levels and 1 .. %d "
                    "features (N = %lld, H = %d, W = %d, levels = %d, max_features = %d)",
                    SKIMI_LENS_MAX_SIDE, SKIMI_CHESS_MAX_PIXELS, SKIMI_ORB_MAX_LEVELS, SKIMI_ORB_MAX_FEATURES, (long long)N, H, W, levels,
                    max_features);
    SKIMI_CHECK_ARG(ch == 1 || ch == 3 || ch == 4, "skimi_orb_features: 1, 3 or 4 channels, got %d", ch);
    SKIMI_CHECK_ARG(threshold >= 0 && threshold <= 254, "skimi_orb_features: threshold must be in 0 .. 254, got %d", threshold);
    SKIMI_CHECK_ARG(ws_bytes >= skimi_orb_workspace_bytes(N, H, W, levels), "skimi_orb_features: workspace too small (%zu < %zu bytes)",
                    ws_bytes, skimi_orb_workspace_bytes(N, H, W, levels));
    SKIMI_CHECK_ARG(((uintptr_t)ws & 15) == 0 && ((uintptr_t)pattern & 3) == 0,
                    "skimi_orb_features: workspace must be 16-byte aligned and the pattern 4-byte aligned");
    py.threshold = threshold;
    OrbWs w;
    orb_ws_layout(N, py, ws, &w);
    hipStream_t st = (hipStream_t)stream;
    const dim3 block(kOrbThreads);
    const long n0 = (long)H * W;
    const dim3 g0((unsigned)cdiv(n0, kOrbThreads), (unsigned)N);
    if (ch == 1)
        hipLaunchKernelGGL(orb_gray_kernel<1>, g0, block, 0, st, frames, n0, py.P, w.gray);
    else if (ch == 3)
        hipLaunchKernelGGL(orb_gray_kernel<3>, g0, block, 0, st, frames, n0, py.P, w.gray);
    else
        hipLaunchKernelGGL(orb_gray_kernel<4>, g0, block, 0, st, frames, n0, py.P, w.gray);
    for (int l = 1; l < py.L; ++l)
        hipLaunchKernelGGL(orb_shrink_kernel, dim3((unsigned)cdiv((long)py.W[l] * py.H[l], kOrbThreads), (unsigned)N), block, 0, st, w.gray,
                           py.P, py.poff[l - 1], py.W[l - 1], py.H[l - 1], py.poff[l], py.W[l], py.H[l]);
    hipLaunchKernelGGL(orb_blur_kernel, dim3((unsigned)cdiv(n0, kOrbThreads), (unsigned)py.L, (unsigned)N), block, 0, st, py,
                       (const unsigned char*)w.gray, w.blur);
    hipLaunchKernelGGL(orb_fast_kernel, dim3((unsigned)(cdiv(W, kFastTW) * cdiv(H, kFastTH)), (unsigned)py.L, (unsigned)N), block, 0, st, py,
                       (const unsigned char*)w.gray, w.score);
    const dim3 groups((unsigned)cdiv(n0, kOrbTile), (unsigned)py.L, (unsigned)N);
    hipLaunchKernelGGL(orb_count_kernel, groups, block, 0, st, py, (const unsigned char*)w.score, roi, w.block_count);
    hipLaunchKernelGGL(orb_write_kernel, groups, block, 0, st, py, (const unsigned char*)w.score, roi, (const unsigned*)w.block_count, w.cand,
                       level_count);
    hipLaunchKernelGGL(orb_harris_kernel, dim3((unsigned)cdiv(py.cap[0], kOrbThreads), (unsigned)py.L, (unsigned)N), block, 0, st, py,
                       (const unsigned char*)w.gray, (const int*)w.cand, (const int*)level_count, w.harris);
    hipLaunchKernelGGL(orb_select_kernel, dim3((unsigned)py.L, (unsigned)N), block, 0, st, py, (const unsigned char*)w.score,
                       (const int*)w.cand, (const long long*)w.harris, (const int*)level_count, xy_level, xy, level, direction, score,
                       reinterpret_cast<long long*>(harris), desc, count);
    const long total = (long)N * py.M;
    hipLaunchKernelGGL(orb_describe_kernel, dim3((unsigned)cdiv(total, kOrbWaves)), block, 0, st, py, (const unsigned char*)w.gray,
                       (const unsigned char*)w.blur, reinterpret_cast<const signed char*>(pattern), (const int*)xy_level, (const int*)level,
                       (const int*)count, total, direction, desc);
    SKIMI_LAUNCH_CHECK();
    return SKIMI_OK;
}

int skimi_match_hamming(const int32_t* d1, const int32_t* n1, int32_t M1, const int32_t* d2, const int32_t* n2, int32_t M2, int64_t B,
                        int32_t cross_check, double ratio, int32_t max_distance, int32_t max_matches, int32_t* pairs, int32_t* dist,
                        int32_t* count, void* stream) {
    SKIMI_CHECK_ARG(d1 && n1 && d2 && n2 && pairs && dist && count, "skimi_match_hamming: null pointer");
    SKIMI_CHECK_ARG(B >= 1 && B <= (1LL << 30), "skimi_match_hamming: need 1 <= B <= 2^30 pairs of sets, got %lld", (long long)B);
    SKIMI_CHECK_ARG(M1 >= 1 && M1 <= SKIMI_ORB_MAX_FEATURES && M2 >= 1 && M2 <= SKIMI_ORB_MAX_FEATURES,
                    "skimi_match_hamming: the sets hold 1 .. %d descriptors, got %d and %d", SKIMI_ORB_MAX_FEATURES, M1, M2);
    SKIMI_CHECK_ARG(max_matches >= 1 && max_matches <= SKIMI_ORB_MAX_FEATURES, "skimi_match_hamming: max_matches must be in 1 .. %d, got %d",
                    SKIMI_ORB_MAX_FEATURES, max_matches);
    SKIMI_CHECK_ARG(ratio == ratio, "skimi_match_hamming: ratio must not be NaN (negative: no ratio test)");
    SKIMI_CHECK_ARG(max_distance <= 256, "skimi_match_hamming: max_distance must be at most 256 (negative: no bound), got %d", max_distance);
    SKIMI_CHECK_ARG(((uintptr_t)d1 & 15) == 0 && ((uintptr_t)d2 & 15) == 0, "skimi_match_hamming: descriptors must be 16-byte aligned");
    hipLaunchKernelGGL(match_hamming_kernel, dim3((unsigned)B), dim3(kMatchThreads), 0, (hipStream_t)stream,
                       reinterpret_cast<const unsigned*>(d1), (const int*)n1, M1, reinterpret_cast<const unsigned*>(d2), (const int*)n2, M2,
                       cross_check, ratio, max_distance, max_matches, pairs, dist, count);
    SKIMI_LAUNCH_CHECK();
    return SKIMI_OK;
}

}  // extern "C"
