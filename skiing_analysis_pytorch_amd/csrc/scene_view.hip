// 3D scene views (DESIGN §2 "Scene views"): clouds of coloured points and an ordered list of depth-tested primitives seen
// from F cameras, one depth test per pixel.  The rules are in include/skimi.h; tests/scene_view_restated.py is the
// restatement.  Depth is one integer w per fragment (larger = nearer, 0 = empty), so the test is exact and the picture is
// bitwise reproducible whatever order the waves run in.
//
// Two passes over a chunk of frames whose key buffer [frames, H, W] u64 fits the workspace:
//  - splat: a thread per (frame, point) projects the point in f64 and writes (w << 32) | index with a 64-bit atomic max into
//    the s x s pixels it covers.  The maximum is the nearest point, among equal w the highest index: no order can change it.
//  - resolve: draw.hip's layout (raster_tiles.h).  A workgroup owns a block of 4 x 4 tiles of 64 x 16 pixels, a thread kPix = 4 adjacent
//    pixels of a row; the primitive list is binned to the block and then to each tile in list order (compact.h's
//    ordered_rank), and every thread runs its pixels over the tile's list starting from the splat key.  A pixel has one
//    owner: no atomics.  A tile that no primitive touches only resolves its keys.
#include <algorithm>

#include "common.h"
#include "compact.h"
#include "exact_int.h"
#include "raster_tiles.h"
#include "warp_u8.h"

#pragma clang fp contract(off)

namespace skimi {

namespace {

constexpr int kThreads = kRasterThreads;
constexpr int kViewWords = 20, kPrimWords = 12;
constexpr double kWOne = (double)SKIMI_SCENE_W_ONE;

// rule 1's clamp: 1 .. 2^30, a NaN gives 1
__device__ __forceinline__ double clamp_w(double q) {
    if (!(q >= 1.0)) q = 1.0;
    if (q > kWOne) q = kWOne;
    return q;
}

// the cloud of global frame f, or -1
__device__ __forceinline__ int cloud_of(const int* __restrict__ cof, int P, long f) {
    const long p = cof ? (long)cof[f] : (P == 1 ? 0 : f);
    return (p >= 0 && p < P) ? (int)p : -1;
}

// ---- splat -------------------------------------------------------------------------------------------------------------------
// grid (ceil(N / kThreads), frames of the chunk); f0: the chunk's first frame; keys: the chunk's buffer, zeroed
__global__ __launch_bounds__(kThreads) void scene_splat_kernel(const double* __restrict__ views, const float* __restrict__ xyz,
                                                               const long long* __restrict__ count,
                                                               const int* __restrict__ cof, int P, long long N, int size, long f0,
                                                               unsigned long long* keys, int H, int W) {
    const long f = f0 + blockIdx.y;
    const int p = cloud_of(cof, P, f);
    if (p < 0) return;
    const long long n = count ? min(max(count[p], 0ll), N) : N;
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const double* __restrict__ V = views + (size_t)f * kViewWords;   // the same in every lane: scalar loads
    const float* __restrict__ q = xyz + ((size_t)p * N + i) * 3;
    const double x = (double)q[0], y = (double)q[1], z = (double)q[2];
    const double X = ((V[0] * x + V[1] * y) + V[2] * z) + V[3];
    const double Y = ((V[4] * x + V[5] * y) + V[6] * z) + V[7];
    const double Z = ((V[8] * x + V[9] * y) + V[10] * z) + V[11];
    if (!(__builtin_isfinite(X) && __builtin_isfinite(Y) && __builtin_isfinite(Z))) return;
    const double near = V[16], far = V[17];
    if (!(Z >= near && Z <= far)) return;
    double u, v, w;
    if (V[18] != 0.0) {
        u = V[12] * X + V[14];
        v = V[13] * Y + V[15];
        w = floor((kWOne * (far - Z)) / (far - near));
    } else {
        if (!(Z > 0.0)) return;
        u = (V[12] * X) / Z + V[14];
        v = (V[13] * Y) / Z + V[15];
        w = floor((kWOne * near) / Z);
    }
    w = clamp_w(w);
    const double fu = floor(u), fv = floor(v);
    // the square's first pixel, still in f64: it meets the frame iff it starts inside (-size, W) x (-size, H); false for a NaN
    const double off = (double)((size - 1) >> 1), ox = fu - off, oy = fv - off;
    if (!(ox > -(double)size && ox < (double)W && oy > -(double)size && oy < (double)H)) return;
    const int px = (int)ox, py = (int)oy;
    const unsigned long long key = ((unsigned long long)(unsigned)(int)w << 32) | (unsigned long long)(unsigned)i;
    unsigned long long* frame = keys + (size_t)blockIdx.y * H * W;
    for (int dy = 0; dy < size; ++dy) {
        const int yy = py + dy;
        if (yy < 0 || yy >= H) continue;
        for (int dx = 0; dx < size; ++dx) {
            const int xx = px + dx;
            if (xx < 0 || xx >= W) continue;
            atomicMax(frame + (size_t)yy * W + xx, key);
        }
    }
}

// ---- resolve + primitives ----------------------------------------------------------------------------------------------------
struct Prim {
    int kind, x0, y0, x1, y1, r, colour, w0, w1;
};

__device__ __forceinline__ int clamp_wi(int w) { return min(max(w, 1), SKIMI_SCENE_W_ONE); }

// a record as rule 3 reads it; a disc is the capsule a -> a
__device__ __forceinline__ Prim read_prim(const int* __restrict__ rec) {
    Prim s;
    s.kind = rec[0];
    s.x0 = sat20(rec[1]), s.y0 = sat20(rec[2]);
    s.x1 = sat20(rec[3]), s.y1 = sat20(rec[4]);
    s.r = sat20(rec[5]);
    s.colour = rec[6];
    s.w0 = clamp_wi(rec[7]), s.w1 = clamp_wi(rec[8]);
    if (s.kind != SKIMI_SCENE_DISC && s.kind != SKIMI_SCENE_CAPSULE) s.kind = SKIMI_SCENE_NONE;
    if (s.kind == SKIMI_SCENE_DISC) s.x1 = s.x0, s.y1 = s.y0, s.w1 = s.w0;
    return s;
}

// can the primitive cover a pixel whose centre lies in [tx0, tx1] x [ty0, ty1] (1/16 pixel)?  Conservative: its extent
// grown by its radius plus one pixel (d <= r needs a true distance below r + 1).
__device__ __forceinline__ bool touches(const Prim& s, int tx0, int ty0, int tx1, int ty1) {
    if (s.kind == SKIMI_SCENE_NONE || s.r < 0) return false;
    const int g = 16 + s.r;
    return min(s.x0, s.x1) - g <= tx1 && max(s.x0, s.x1) + g >= tx0 && min(s.y0, s.y1) - g <= ty1 && max(s.y0, s.y1) + g >= ty0;
}

// The fragment of s at the pixel whose centre is (16 u, 16 v): its w, or 0 where the centre is not covered.  root:
// isqrt(|b - a|^2).  The depth along a capsule is w0 + sign floor(m t / L2) with m = |w1 - w0| < 2^30 and 0 < t < L2 <= 2^43: the
// product does not fit a double, so m goes through the division a byte at a time from the top (long division in base
// 256): acc = 256 rem + digit t < 2^51 + 2^51 stays exact, and so does every quotient.
__device__ __forceinline__ int fragment(const Prim& s, double root, int u, int v) {
    const double px = (double)(16 * u - s.x0), py = (double)(16 * v - s.y0);   // p - a
    if (!(root > 0.0)) return isqrt_exact(px * px + py * py) <= (double)s.r ? s.w0 : 0;
    const double ex = (double)(s.x1 - s.x0), ey = (double)(s.y1 - s.y0);       // b - a
    const double t = px * ex + py * ey, L2 = ex * ex + ey * ey;
    if (t <= 0.0) return isqrt_exact(px * px + py * py) <= (double)s.r ? s.w0 : 0;
    if (t >= L2) {
        const double qx = px - ex, qy = py - ey;
        return isqrt_exact(qx * qx + qy * qy) <= (double)s.r ? s.w1 : 0;
    }
    if (floor_div_exact(fabs(px * ey - py * ex), root) > (double)s.r) return 0;
    const int m = abs(s.w1 - s.w0);
    double rem = 0.0, Q = 0.0;
#pragma unroll
    for (int k = 3; k >= 0; --k) {
        const double acc = rem * 256.0 + (double)((m >> (8 * k)) & 255) * t;
        const double q = floor_div_exact(acc, L2);
        rem = acc - q * L2;
        Q = Q * 256.0 + q;
    }
    return s.w1 >= s.w0 ? s.w0 + (int)Q : s.w0 - (int)Q;
}

// grid (ceil(W / kBlockW), ceil(H / kBlockH), frames of the chunk); keys: the chunk's buffer; everything else is indexed by
// the global frame f0 + blockIdx.z
__global__ __launch_bounds__(kThreads) void scene_resolve_kernel(const unsigned long long* __restrict__ keys,
                                                                 const double* __restrict__ views, const unsigned char* __restrict__ rgb,
                                                                 const int* __restrict__ cof, int P, long long N,
                                                                 const int* __restrict__ prims, int prim_axes, int M,
                                                                 const unsigned char* background, unsigned bg_colour, unsigned char* out,
                                                                 float* __restrict__ depth, int* __restrict__ index, long f0, int H,
                                                                 int W, int aligned) {
    __shared__ unsigned short s_block[SKIMI_SCENE_MAX_PRIMS], s_list[SKIMI_SCENE_MAX_PRIMS];
    __shared__ unsigned s_wtot[2][kThreads / 64];
    const int tid = threadIdx.x;
    const long f = f0 + blockIdx.z;
    const int* __restrict__ recs = prims + (prim_axes == 3 ? (size_t)f * M * kPrimWords : 0);
    const int bx0 = blockIdx.x * kBlockW, by0 = blockIdx.y * kBlockH;   // inside the frame
    const size_t pixels = (size_t)H * W;
    const unsigned long long* __restrict__ kf = keys + (size_t)blockIdx.z * pixels;
    const int cloud = cloud_of(cof, P, f);
    const unsigned char* __restrict__ colours = rgb + (size_t)max(cloud, 0) * N * 3;   // read only where a key is set
    const double* __restrict__ V = views + (size_t)f * kViewWords;
    const double near = V[16], far = V[17];
    const bool ortho = V[18] != 0.0;

    // the block's list, in list order: a primitive a thread, a round of kThreads at a time
    unsigned nb = 0;
    int buf = 0;
    {
        const int x1 = 16 * (min(bx0 + kBlockW, W) - 1), y1 = 16 * (min(by0 + kBlockH, H) - 1);
        for (int i0 = 0; i0 < M; i0 += kThreads) {   // uniform trip count: every thread reaches the barrier
            const int i = i0 + tid;
            const bool kept = i < M && touches(read_prim(recs + (size_t)i * kPrimWords), 16 * bx0, 16 * by0, x1, y1);
            list_round(kept, i, s_block, nb, s_wtot, buf);
        }
    }
    if (nb) __syncthreads();       // s_block

    for (int t = 0; t < kTilesX * kTilesY; ++t) {   // the block's tiles; everything that skips one is workgroup-uniform
        const int px0 = bx0 + (t % kTilesX) * kTileW, py0 = by0 + (t / kTilesX) * kTileH;
        if (px0 >= W || py0 >= H) continue;
        // the tile's list out of the block's, order kept.  The barrier inside the first round is also what keeps this
        // tile's writes to s_list behind every thread's reads of the tile before.
        unsigned n = 0;
        if (nb) {
            const int tx1 = 16 * (min(px0 + kTileW, W) - 1), ty1 = 16 * (min(py0 + kTileH, H) - 1);
            for (unsigned i0 = 0; i0 < nb; i0 += kThreads) {
                const unsigned i = i0 + tid;
                const int idx = i < nb ? (int)s_block[i] : 0;
                const bool kept = i < nb && touches(read_prim(recs + (size_t)idx * kPrimWords), 16 * px0, 16 * py0, tx1, ty1);
                list_round(kept, idx, s_list, n, s_wtot, buf);
            }
            __syncthreads();       // s_list
        }

        const int v = py0 + tid / kSpanX;
        const int u0 = px0 + (tid % kSpanX) * kPix;
        if (v >= H || u0 >= W) continue;   // this thread owns no pixel of the tile; it still takes part in the next tile's barriers
        const size_t at = (size_t)v * W + u0;
        const size_t fat = (size_t)f * pixels + at;
        unsigned int words[3];
        if (background) {
            span_load<3>(background + fat * 3, words, aligned, u0, W);
        } else {
            // 4 pixels of c0 c1 c2 as three dwords
            const unsigned c0 = bg_colour & 255u, c1 = (bg_colour >> 8) & 255u, c2 = (bg_colour >> 16) & 255u;
            words[0] = c0 | (c1 << 8) | (c2 << 16) | (c0 << 24);
            words[1] = c1 | (c2 << 8) | (c0 << 16) | (c1 << 24);
            words[2] = c2 | (c0 << 8) | (c1 << 16) | (c2 << 24);
        }
        int bw[kPix], bi[kPix];
        unsigned bc[kPix];
#pragma unroll
        for (int p = 0; p < kPix; ++p) {
            bw[p] = 0, bi[p] = -1, bc[p] = 0;
            if (u0 + p >= W) continue;
            const unsigned long long key = kf[at + p];
            if (key) {
                bw[p] = (int)(key >> 32);
                bi[p] = (int)(unsigned)key;
                const unsigned char* c = colours + (size_t)(unsigned)key * 3;
                bc[p] = (unsigned)c[0] | ((unsigned)c[1] << 8) | ((unsigned)c[2] << 16);
            }
        }
        for (unsigned k = 0; k < n; ++k) {
            const int idx = __builtin_amdgcn_readfirstlane((int)s_list[k]);   // the same in every lane: scalar record loads
            const Prim s = read_prim(recs + (size_t)idx * kPrimWords);
            if (!touches(s, 16 * u0, 16 * v, 16 * (u0 + kPix - 1), 16 * v)) continue;   // not on this thread's span
            const double ex = (double)(s.x1 - s.x0), ey = (double)(s.y1 - s.y0);
            const double root = isqrt_exact(ex * ex + ey * ey);   // 0 iff a = b: the disc
#pragma unroll
            for (int p = 0; p < kPix; ++p) {
                if (u0 + p >= W) continue;
                const int w = fragment(s, root, u0 + p, v);
                if (w && w >= bw[p]) bw[p] = w, bc[p] = (unsigned)s.colour & 0xFFFFFFu;
            }
        }
#pragma unroll
        for (int p = 0; p < kPix; ++p) {
            if (u0 + p >= W) continue;
            if (bw[p]) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int byte = p * 3 + c, sh = 8 * (byte & 3);
                    words[byte >> 2] = (words[byte >> 2] & ~(255u << sh)) | (((bc[p] >> (8 * c)) & 255u) << sh);
                }
            }
            if (depth) {
                double Z = __builtin_inf();
                if (bw[p]) Z = ortho ? far - ((double)bw[p] * (far - near)) / kWOne : (kWOne * near) / (double)bw[p];
                depth[fat + p] = (float)Z;
            }
            if (index) index[fat + p] = bi[p];
        }
        warp_store<3>(out + fat * 3, words, aligned, u0, W);
    }
}

}  // namespace

}  // namespace skimi

using namespace skimi;

extern "C" {

size_t skimi_scene_view_workspace_bytes(int64_t F, int32_t H, int32_t W, size_t cap_bytes) {
    if (F < 1 || H < 1 || W < 1) return 0;
    const size_t per = (size_t)H * W * 8;
    size_t frames = (size_t)F;
    if (cap_bytes) frames = std::min(frames, std::max<size_t>(1, cap_bytes / per));
    return per * frames;
}

int skimi_scene_view_render(const double* views, const float* xyz, const uint8_t* rgb, const int64_t* count,
                            const int32_t* cloud_of_frame, int32_t P, int64_t N, int32_t point_size, const int32_t* prims,
                            int32_t prim_axes, int32_t M, const uint8_t* background, uint32_t bg_colour, uint8_t* frames, float* depth,
                            int32_t* index, int64_t F, int32_t H, int32_t W, void* ws, size_t ws_bytes, void* stream) {
    SKIMI_CHECK_ARG(F >= 1 && F < (1ll << 31), "skimi_scene_view_render: F = %lld outside 1 .. 2^31 - 1", (long long)F);
    SKIMI_CHECK_ARG(H >= 1 && W >= 1 && H <= SKIMI_LENS_MAX_SIDE && W <= SKIMI_LENS_MAX_SIDE,
                    "skimi_scene_view_render: frame %d x %d outside 1 .. %d a side", W, H, SKIMI_LENS_MAX_SIDE);
    SKIMI_CHECK_ARG(P >= 0 && N >= 0 && N < (1ll << 31), "skimi_scene_view_render: P = %d, N = %lld outside 0 <= P, 0 <= N < 2^31", P,
                    (long long)N);
    SKIMI_CHECK_ARG(point_size >= 1 && point_size <= SKIMI_SCENE_MAX_POINT_SIZE, "skimi_scene_view_render: point_size = %d outside 1 .. %d",
                    point_size, SKIMI_SCENE_MAX_POINT_SIZE);
    SKIMI_CHECK_ARG(M >= 0 && M <= SKIMI_SCENE_MAX_PRIMS, "skimi_scene_view_render: M = %d outside 0 .. %d", M, SKIMI_SCENE_MAX_PRIMS);
    SKIMI_CHECK_ARG(prim_axes == 2 || prim_axes == 3, "skimi_scene_view_render: prim_axes = %d (2: [M, 12], 3: [F, M, 12])", prim_axes);
    SKIMI_CHECK_ARG(cloud_of_frame || P <= 1 || P == F, "skimi_scene_view_render: %d clouds for %lld frames need cloud_of_frame", P,
                    (long long)F);
    const bool cloud = P >= 1 && N >= 1;
    SKIMI_CHECK_ARG(views && frames && ws && (prims || M == 0) && (!cloud || (xyz && rgb)),
                    "skimi_scene_view_render: NULL views, frames, ws, prims or cloud");
    const size_t pixels = (size_t)H * W, per = pixels * 8;
    if (ws_bytes < per) {
        set_error("skimi_scene_view_render: workspace of %zu bytes, one frame needs %zu", ws_bytes, per);
        return SKIMI_ERR_WORKSPACE;
    }
    const int64_t chunk = std::min<int64_t>(std::min<int64_t>(F, (int64_t)(ws_bytes / per)), 65535);
    const int aligned = ((int64_t)W * 3) % 4 == 0 && ((uintptr_t)frames & 3) == 0 && ((uintptr_t)background & 3) == 0;
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* keys = (unsigned long long*)ws;
    for (int64_t f0 = 0; f0 < F; f0 += chunk) {
        const int64_t n = std::min(chunk, F - f0);
        SKIMI_HIP(hipMemsetAsync(keys, 0, per * (size_t)n, st));
        if (cloud) {
            const dim3 grid((unsigned)cdiv(N, kThreads), (unsigned)n);
            hipLaunchKernelGGL(scene_splat_kernel, grid, dim3(kThreads), 0, st, views, xyz, (const long long*)count, cloud_of_frame, P,
                               (long long)N, point_size, (long)f0, keys, H, W);
            SKIMI_LAUNCH_CHECK();
        }
        const dim3 grid((unsigned)cdiv(W, kBlockW), (unsigned)cdiv(H, kBlockH), (unsigned)n);
        hipLaunchKernelGGL(scene_resolve_kernel, grid, dim3(kThreads), 0, st, keys, views, rgb, cloud ? cloud_of_frame : nullptr,
                           cloud ? P : 0, (long long)N, prims, prim_axes, M, background, bg_colour, frames, depth, index, (long)f0, H, W,
                           aligned);
        SKIMI_LAUNCH_CHECK();
    }
    return SKIMI_OK;
}

}  // extern "C"
