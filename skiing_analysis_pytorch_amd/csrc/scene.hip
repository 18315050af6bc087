// The filtered, coloured point cloud of a VGGT time step (predictions_to_glb, vggt/visual_util.py:39-236, which runs
// in NumPy on the host), on device so that only the kept vertices cross to the host:
//   colours            (:170)      uint8 = trunc(float32(v) * 255)
//   threshold          (:172-179)  the conf_thres-th percentile of the scene's confidences
//   mask + compaction  (:179-192)  conf >= thr, conf > 1e-5, optional black / white background masks; pixel order
//   scene scale        (:199-204)  the 5th / 95th percentile box of the kept vertices
//   alignment          (:284-305)  A = E0^-1 diag(-1, -1, 1, 1)
// Rules where NumPy's result depends on its implementation or version: DESIGN §2 "Scene cloud".
//
// A scene is n = S H W pixels; all B scenes go through every launch (scene = blockIdx.y), a workgroup owns `tile`
// consecutive pixels of one scene.  Every percentile is an exact selection: a radix select over the order-preserving
// 32-bit key (fp64_util.h's key32), four passes of 8 bits, one launch per pass.  A pass histograms in LDS and adds its bins
// to the scene's global histogram; the NEXT launch starts by resolving that histogram (every workgroup does it for
// itself and gets the same digit), so there is no launch between passes.  Both order statistics of a percentile (ranks
// i and i + 1) and, for the scale, both percentiles of an axis are selected in the same passes: selections of one key
// stream that still share their prefix share one histogram.  The mask pass counts the kept pixels per workgroup; the
// first vertex pass turns the counts into offsets and writes the cloud in pixel order (compact.h).  Ten launches
// whatever the data; no floating-point sum anywhere, only integer atomics (order-independent): results are bitwise
// reproducible and a scene's results do not depend on the batch around it.
#include <math.h>

#include "common.h"
#include "compact.h"
#include "fp64_util.h"
#include "reduce.h"

namespace skimi {

constexpr int kSceneThreads = 256;
constexpr int kSceneWaves = kSceneThreads / 64;
constexpr long kSceneMinTile = 4096;     // pixels of a workgroup: 16 per thread
constexpr long kSceneMaxGroups = 1024;   // workgroups per scene (a workgroup sums this many counts for its offset)
constexpr long kSceneMaxN = 2147483647L / 3;
constexpr int kConfSel = 2;    // ranks i, i + 1 of the threshold percentile
constexpr int kXyzSel = 12;    // per axis: ranks i, i + 1 of the 5th and of the 95th percentile
constexpr int kXyzGroup = 4;

static inline long scene_tile(long n) {
    const long t = cdiv(cdiv(n, kSceneMaxGroups), kSceneMinTile) * kSceneMinTile;
    return t < kSceneMinTile ? kSceneMinTile : t;
}

// per scene, followed by block_count[groups]
struct SceneWs {
    double thr[4];   // thr, lo, hi
    unsigned conf_hist[4][kConfSel][256];
    unsigned xyz_hist[4][kXyzSel][256];
    unsigned conf_state[4][kConfSel][2];   // after pass p: prefix, rank among the keys that share it
    unsigned xyz_state[4][kXyzSel][2];
    unsigned n_nan_conf, n_nonfinite, n_nan_axis[3], count, pad[2];
};
static_assert(sizeof(SceneWs) % 8 == 0, "scenes are laid out back to back");

static inline size_t scene_ws_stride(long n) { return align_up(sizeof(SceneWs) + (size_t)cdiv(n, scene_tile(n)) * 4, 8); }

__device__ inline unsigned char colour_u8(float v) {
    const float p = v * 255.0f;
    if (!(p >= 0.0f)) return 0;   // NaN, negative
    if (p >= 256.0f) return 255;
    return (unsigned char)(int)p;
}

struct SceneImage {
    const float* img;   // this scene's images
    int nchw, hw;
    int black, white;
};
__device__ inline void scene_colour(const SceneImage& im, int p, unsigned char (&c)[3]) {
    if (im.nchw) {
        const int s = p / im.hw, r = p - s * im.hw;
        const float* q = im.img + (long)s * 3 * im.hw + r;
#pragma unroll
        for (int k = 0; k < 3; ++k) c[k] = colour_u8(q[(long)k * im.hw]);
    } else {
#pragma unroll
        for (int k = 0; k < 3; ++k) c[k] = colour_u8(im.img[(long)p * 3 + k]);
    }
}
__device__ inline bool scene_kept(const SceneImage& im, int p, float cf, double thr) {
    if (!((double)cf >= thr && cf > 1e-5f)) return false;
    if (im.black | im.white) {
        unsigned char c[3];
        scene_colour(im, p, c);
        if (im.black && (int)c[0] + c[1] + c[2] < 16) return false;
        if (im.white && c[0] > 240 && c[1] > 240 && c[2] > 240) return false;
    }
    return true;
}

// ---- the shared radix select: NSEL selections in groups of GRP over one key stream each ----
// A selection's leader is the first selection of its group with the same prefix: only leaders histogram.
template <int NSEL, int GRP>
__device__ inline void sel_leaders(const unsigned* s_prefix, unsigned* s_leader) {
    const int j = threadIdx.x;
    if (j < NSEL) {
        int l = j;
        for (int k = j / GRP * GRP; k < j; ++k)
            if (s_prefix[k] == s_prefix[j]) {
                l = k;
                break;
            }
        s_leader[j] = (unsigned)l;
    }
}

// Start of pass P (0..3), or P = 4 for the result: brings s_prefix / s_rank / s_leader to the state before pass P by
// resolving pass P - 1's global histogram, and clears the LDS histogram.  For P <= 1 the caller has put prefix 0 and
// the ranks into s_prefix / s_rank.  The writer workgroup records the state after pass P - 1 for the launches that follow.
template <int NSEL, int GRP>
__device__ inline void sel_begin(int P, const unsigned* ghist, unsigned* gstate, bool writer, unsigned* h, unsigned* s_prefix,
                                 unsigned* s_rank, unsigned* s_leader) {
    const int tid = threadIdx.x;
    if (P >= 2 && tid < NSEL) {
        s_prefix[tid] = gstate[((P - 2) * NSEL + tid) * 2];
        s_rank[tid] = gstate[((P - 2) * NSEL + tid) * 2 + 1];
    }
    __syncthreads();
    sel_leaders<NSEL, GRP>(s_prefix, s_leader);
    if (P >= 1) {
        const unsigned* gh = ghist + (P - 1) * NSEL * 256;
        for (int i = tid; i < NSEL * 256; i += kSceneThreads) h[i] = gh[i];
        __syncthreads();
        if (tid < NSEL) {
            const unsigned* hh = h + s_leader[tid] * 256;
            unsigned r = s_rank[tid], b = 0;
            while (b < 255 && r >= hh[b]) r -= hh[b++];
            const unsigned prefix = s_prefix[tid] | (b << (32 - 8 * P));
            s_prefix[tid] = prefix;
            s_rank[tid] = r;
            if (writer) {
                gstate[((P - 1) * NSEL + tid) * 2] = prefix;
                gstate[((P - 1) * NSEL + tid) * 2 + 1] = r;
            }
        }
        __syncthreads();
        sel_leaders<NSEL, GRP>(s_prefix, s_leader);
    }
    __syncthreads();
    for (int i = tid; i < NSEL * 256; i += kSceneThreads) h[i] = 0;
    __syncthreads();
}

// one key of group j0 / GRP into the histograms of that group's leaders, pass P
template <int GRP>
__device__ inline void sel_add(int P, unsigned key, int j0, unsigned* h, const unsigned* s_prefix, const unsigned* s_leader) {
    const unsigned hi_mask = P == 0 ? 0u : 0xFFFFFFFFu << (32 - 8 * P);
    const unsigned digit = (key >> (24 - 8 * P)) & 255u;
#pragma unroll
    for (int k = 0; k < GRP; ++k) {
        const int j = j0 + k;
        if (s_leader[j] == (unsigned)j && (key & hi_mask) == s_prefix[j]) atomicAdd(&h[j * 256 + digit], 1u);
    }
}

template <int NSEL>
__device__ inline void sel_flush(const unsigned* h, unsigned* ghist_pass) {
    __syncthreads();
    for (int i = threadIdx.x; i < NSEL * 256; i += kSceneThreads)
        if (h[i]) atomicAdd(&ghist_pass[i], h[i]);
}

// ---- launch 1: clear the workspace, A = E0^-1 diag(-1, -1, 1, 1) ----
__global__ __launch_bounds__(kSceneThreads) void scene_init_kernel(const float* __restrict__ extrinsic, int S, char* ws,
                                                                   size_t ws_stride, double* __restrict__ transform) {
    const long b = blockIdx.x;
    unsigned* w = reinterpret_cast<unsigned*>(ws + b * ws_stride);
    for (size_t i = threadIdx.x; i < ws_stride / 4; i += kSceneThreads) w[i] = 0;
    if (threadIdx.x != 0) return;
    const float* e = extrinsic + b * S * 12;
    double m[3][3], t[3];
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) m[r][c] = (double)e[r * 4 + c];
        t[r] = (double)e[r * 4 + 3];
    }
    // general inverse by the adjugate (np.linalg.inv does not assume a rotation)
    const double c00 = m[1][1] * m[2][2] - m[1][2] * m[2][1];
    const double c01 = m[1][2] * m[2][0] - m[1][0] * m[2][2];
    const double c02 = m[1][0] * m[2][1] - m[1][1] * m[2][0];
    const double det = m[0][0] * c00 + m[0][1] * c01 + m[0][2] * c02;
    double inv[3][3];
    inv[0][0] = c00 / det;
    inv[1][0] = c01 / det;
    inv[2][0] = c02 / det;
    inv[0][1] = (m[0][2] * m[2][1] - m[0][1] * m[2][2]) / det;
    inv[1][1] = (m[0][0] * m[2][2] - m[0][2] * m[2][0]) / det;
    inv[2][1] = (m[0][1] * m[2][0] - m[0][0] * m[2][1]) / det;
    inv[0][2] = (m[0][1] * m[1][2] - m[0][2] * m[1][1]) / det;
    inv[1][2] = (m[0][2] * m[1][0] - m[0][0] * m[1][2]) / det;
    inv[2][2] = (m[0][0] * m[1][1] - m[0][1] * m[1][0]) / det;
    double* A = transform + b * 16;
    for (int r = 0; r < 3; ++r) {
        A[r * 4 + 0] = -inv[r][0];
        A[r * 4 + 1] = -inv[r][1];
        A[r * 4 + 2] = inv[r][2];
        A[r * 4 + 3] = -(inv[r][0] * t[0] + inv[r][1] * t[1] + inv[r][2] * t[2]);
    }
    A[12] = 0.0;
    A[13] = 0.0;
    A[14] = 0.0;
    A[15] = 1.0;
}

// ---- launches 2-5: pass P of the threshold's select over the confidences; pass 0 counts the NaNs ----
template <int P>
__global__ __launch_bounds__(kSceneThreads) void scene_conf_pass_kernel(const float* __restrict__ conf, int n, long tile, double q,
                                                                        char* ws, size_t ws_stride) {
    __shared__ unsigned h[kConfSel * 256];
    __shared__ unsigned s_prefix[kConfSel], s_rank[kConfSel], s_leader[kConfSel];
    const int tid = threadIdx.x;
    const long b = blockIdx.y, g = blockIdx.x;
    SceneWs* w = reinterpret_cast<SceneWs*>(ws + b * ws_stride);
    if (P <= 1 && tid < kConfSel) {
        const PctPos pos = pct_pos(q, (unsigned)n);
        s_prefix[tid] = 0;
        s_rank[tid] = tid ? pos.i1 : pos.i0;
    }
    sel_begin<kConfSel, kConfSel>(P, &w->conf_hist[0][0][0], &w->conf_state[0][0][0], g == 0, h, s_prefix, s_rank, s_leader);
    const float* c = conf + b * n;
    const long beg = g * tile, end = min(beg + tile, (long)n);
    unsigned n_nan = 0;
    for (long i = beg + tid; i < end; i += kSceneThreads) {
        const float v = c[i];
        if (P == 0 && v != v) ++n_nan;
        sel_add<kConfSel>(P, key32(v), 0, h, s_prefix, s_leader);
    }
    sel_flush<kConfSel>(h, &w->conf_hist[P][0][0]);
    if (P == 0) {
        n_nan = wave_sum(n_nan);
        if ((tid & 63) == 0 && n_nan) atomicAdd(&w->n_nan_conf, n_nan);
    }
}

// ---- launch 6: the threshold; kept pixels per workgroup; top byte of the kept vertices' keys; NaN / non-finite counts ----
__global__ __launch_bounds__(kSceneThreads) void scene_mask_kernel(const float* __restrict__ points, const float* __restrict__ conf,
                                                                   const float* __restrict__ images, int n, int hw, long tile,
                                                                   double q, int nchw, int black, int white, char* ws,
                                                                   size_t ws_stride) {
    __shared__ unsigned h[kXyzSel * 256];
    __shared__ unsigned s_prefix[kXyzSel], s_rank[kXyzSel], s_leader[kXyzSel];
    __shared__ unsigned s_cnt[5];
    __shared__ double s_thr;
    const int tid = threadIdx.x;
    const long b = blockIdx.y, g = blockIdx.x;
    SceneWs* w = reinterpret_cast<SceneWs*>(ws + b * ws_stride);
    unsigned* block_count = reinterpret_cast<unsigned*>(w + 1);
    sel_begin<kConfSel, kConfSel>(4, &w->conf_hist[0][0][0], &w->conf_state[0][0][0], g == 0, h, s_prefix, s_rank, s_leader);
    if (tid == 0) {
        const double nan = qnan();
        double lo = (double)unkey32(s_prefix[0]), hi = (double)unkey32(s_prefix[1]);
        double thr = pct_lerp(lo, hi, pct_pos(q, (unsigned)n).gamma);
        if (w->n_nan_conf) thr = lo = hi = nan;   // np.percentile of an array with a NaN
        if (q == 0.0) thr = 0.0;                  // conf_thres == 0: no percentile is taken
        s_thr = thr;
        if (g == 0) {
            w->thr[0] = thr;
            w->thr[1] = lo;
            w->thr[2] = hi;
        }
    }
    __syncthreads();
    const double thr = s_thr;
    for (int i = tid; i < kXyzSel * 256; i += kSceneThreads) h[i] = 0;
    if (tid < kXyzSel) {
        s_prefix[tid] = 0;
        s_leader[tid] = tid / kXyzGroup * kXyzGroup;
    }
    if (tid < 5) s_cnt[tid] = 0;
    __syncthreads();
    const float* c = conf + b * n;
    const float* pts = points + b * n * 3;
    SceneImage im{images + b * n * 3, nchw, hw, black, white};
    const long beg = g * tile, end = min(beg + tile, (long)n);
    unsigned cnt[5] = {0, 0, 0, 0, 0};   // kept, non-finite, NaN x / y / z
    for (long i = beg + tid; i < end; i += kSceneThreads) {
        if (!scene_kept(im, (int)i, c[i], thr)) continue;
        ++cnt[0];
        bool finite = true;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float v = pts[i * 3 + a];
            finite = finite && isfinite(v);
            if (v != v) ++cnt[2 + a];
            sel_add<kXyzGroup>(0, key32(v), a * kXyzGroup, h, s_prefix, s_leader);
        }
        if (!finite) ++cnt[1];
    }
    sel_flush<kXyzSel>(h, &w->xyz_hist[0][0][0]);
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const unsigned v = wave_sum(cnt[k]);
        if ((tid & 63) == 0 && v) atomicAdd(&s_cnt[k], v);
    }
    __syncthreads();
    if (tid == 0) {
        block_count[g] = s_cnt[0];
        if (s_cnt[1]) atomicAdd(&w->n_nonfinite, s_cnt[1]);
        for (int a = 0; a < 3; ++a)
            if (s_cnt[2 + a]) atomicAdd(&w->n_nan_axis[a], s_cnt[2 + a]);
    }
}

// ---- launches 7-9: pass P = 1..3 of the twelve vertex selections; pass 1 also writes the cloud in pixel order ----
template <int P>
__global__ __launch_bounds__(kSceneThreads) void scene_xyz_pass_kernel(const float* __restrict__ points, const float* __restrict__ conf,
                                                                       const float* __restrict__ images, int n, int hw, long tile,
                                                                       int nchw, int black, int white, int align, long cap,
                                                                       const double* __restrict__ transform, char* ws,
                                                                       size_t ws_stride, float* __restrict__ xyz,
                                                                       unsigned char* __restrict__ rgb) {
    __shared__ unsigned h[kXyzSel * 256];
    __shared__ unsigned s_prefix[kXyzSel], s_rank[kXyzSel], s_leader[kXyzSel];
    __shared__ unsigned s_total, s_offset;
    __shared__ unsigned s_wtot[2][kSceneWaves];
    const int tid = threadIdx.x;
    const long b = blockIdx.y, g = blockIdx.x;
    SceneWs* w = reinterpret_cast<SceneWs*>(ws + b * ws_stride);
    const unsigned* block_count = reinterpret_cast<const unsigned*>(w + 1);
    const double thr = w->thr[0];
    if (P == 1) {
        // the scene's kept count and the rows ahead of this workgroup's; integer sums, any order
        group_offsets<kSceneThreads>(block_count, (int)gridDim.x, g, s_total, s_offset);
        const unsigned count = s_total;
        if (g == 0 && tid == 0) w->count = count;
        if (tid < kXyzSel) {
            unsigned rank = 0;
            if (count > 0) {
                const PctPos pos = pct_pos((tid % kXyzGroup) < 2 ? 5.0 : 95.0, count);
                rank = (tid & 1) ? pos.i1 : pos.i0;
            }
            s_prefix[tid] = 0;
            s_rank[tid] = rank;
        }
    }
    sel_begin<kXyzSel, kXyzGroup>(P, &w->xyz_hist[0][0][0], &w->xyz_state[0][0][0], g == 0, h, s_prefix, s_rank, s_leader);
    const float* c = conf + b * n;
    const float* pts = points + b * n * 3;
    SceneImage im{images + b * n * 3, nchw, hw, black, white};
    const long beg = g * tile, end = min(beg + tile, (long)n);
    double A[12];
    if (P == 1 && align)
        for (int k = 0; k < 12; ++k) A[k] = transform[b * 16 + k];
    long row0 = P == 1 ? (long)s_offset : 0;   // rows of this scene ahead of the chunk
    int buf = 0;
    for (long i0 = beg; i0 < end; i0 += kSceneThreads) {   // uniform trip count: the chunk's barrier is reached by all
        const long i = i0 + tid;
        const bool kept = i < end && scene_kept(im, (int)i, c[i], thr);
        float v[3] = {0.f, 0.f, 0.f};
        if (kept) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                v[a] = pts[i * 3 + a];
                sel_add<kXyzGroup>(P, key32(v[a]), a * kXyzGroup, h, s_prefix, s_leader);
            }
        }
        if (P == 1) {
            unsigned chunk;
            const unsigned rank = ordered_rank<kSceneWaves>(kept, s_wtot[buf], chunk);
            if (kept) {
                const long row = row0 + rank;
                if (row < cap) {
                    float* o = xyz + (b * cap + row) * 3;
                    if (align) {
#pragma unroll
                        for (int r = 0; r < 3; ++r)
                            o[r] = (float)(A[r * 4 + 0] * (double)v[0] + A[r * 4 + 1] * (double)v[1] + A[r * 4 + 2] * (double)v[2] +
                                           A[r * 4 + 3]);
                    } else {
                        o[0] = v[0];
                        o[1] = v[1];
                        o[2] = v[2];
                    }
                    unsigned char col[3];
                    scene_colour(im, (int)i, col);
                    unsigned char* oc = rgb + (b * cap + row) * 3;
                    oc[0] = col[0];
                    oc[1] = col[1];
                    oc[2] = col[2];
                }
            }
            row0 += chunk;
            buf ^= 1;   // the next chunk writes the other totals: one barrier per chunk
        }
    }
    sel_flush<kXyzSel>(h, &w->xyz_hist[P][0][0]);
}

// ---- launch 10: the twelve order statistics -> lower, upper, scale; the stats record ----
// stats [B, 16] = thr, lo, hi, n_nan_conf, n_nonfinite, lower xyz, upper xyz, scale, count
__global__ __launch_bounds__(kSceneThreads) void scene_finish_kernel(char* ws, size_t ws_stride, double* __restrict__ stats,
                                                                     long long* __restrict__ count_out) {
    __shared__ unsigned h[kXyzSel * 256];
    __shared__ unsigned s_prefix[kXyzSel], s_rank[kXyzSel], s_leader[kXyzSel];
    const long b = blockIdx.x;
    SceneWs* w = reinterpret_cast<SceneWs*>(ws + b * ws_stride);
    sel_begin<kXyzSel, kXyzGroup>(4, &w->xyz_hist[0][0][0], &w->xyz_state[0][0][0], true, h, s_prefix, s_rank, s_leader);
    if (threadIdx.x != 0) return;
    const double nan = qnan();
    const unsigned count = w->count;
    double* out = stats + b * 16;
    out[0] = w->thr[0];
    out[1] = w->thr[1];
    out[2] = w->thr[2];
    out[3] = (double)w->n_nan_conf;
    out[4] = (double)w->n_nonfinite;
    double sq = 0.0;
    for (int a = 0; a < 3; ++a) {
        double lower = nan, upper = nan;
        if (count > 0 && w->n_nan_axis[a] == 0) {
            const unsigned* p = s_prefix + a * kXyzGroup;
            lower = pct_lerp((double)unkey32(p[0]), (double)unkey32(p[1]), pct_pos(5.0, count).gamma);
            upper = pct_lerp((double)unkey32(p[2]), (double)unkey32(p[3]), pct_pos(95.0, count).gamma);
        }
        out[5 + a] = lower;
        out[8 + a] = upper;
        const double d = upper - lower;
        sq += d * d;
    }
    out[11] = count > 0 ? sqrt(sq) : 1.0;   // the reference's empty-scene value
    out[12] = (double)count;
    out[13] = 0.0;
    out[14] = 0.0;
    out[15] = 0.0;
    count_out[b] = (long long)count;
}

}  // namespace skimi

using namespace skimi;

extern "C" {

int64_t skimi_scene_tile(int64_t n) { return n >= 1 && n <= kSceneMaxN ? scene_tile(n) : 0; }

size_t skimi_scene_workspace_bytes(int64_t B, int64_t n) {
    if (B < 1 || n < 1 || n > kSceneMaxN) return 0;
    return (size_t)B * scene_ws_stride(n);
}

int skimi_scene_cloud(const float* points, const float* conf, const float* images, const float* extrinsic, int64_t B, int32_t S,
                      int32_t H, int32_t W, int32_t images_nchw, double conf_thres, int32_t mask_black_bg, int32_t mask_white_bg,
                      int32_t align, int64_t cap, void* workspace, float* xyz, uint8_t* rgb, int64_t* count, double* stats,
                      double* transform, void* stream) {
    SKIMI_CHECK_ARG(points && conf && images && extrinsic && workspace && xyz && rgb && count && stats && transform,
                    "skimi_scene_cloud: null pointer");
    SKIMI_CHECK_ARG(B >= 1 && B <= 65535 && S >= 1 && H >= 1 && W >= 1,
                    "skimi_scene_cloud: need 1 <= B <= 65535 scenes, S >= 1 views and a non-empty map (B = %lld, S = %d, H = %d, W = %d)",
                    (long long)B, S, H, W);
    const int64_t n = (int64_t)S * H * W;
    SKIMI_CHECK_ARG(n <= kSceneMaxN, "skimi_scene_cloud: a scene holds at most (2^31 - 1) / 3 pixels, got %lld", (long long)n);
    SKIMI_CHECK_ARG(conf_thres >= 0.0 && conf_thres <= 100.0, "skimi_scene_cloud: conf_thres must be in [0, 100], got %g", conf_thres);
    SKIMI_CHECK_ARG(cap >= 1, "skimi_scene_cloud: capacity must be at least 1, got %lld", (long long)cap);
    hipStream_t st = (hipStream_t)stream;
    const long tile = scene_tile(n);
    const size_t stride = scene_ws_stride(n);
    const dim3 grid((unsigned)cdiv(n, tile), (unsigned)B), block(kSceneThreads);
    char* ws = static_cast<char*>(workspace);
    const int hw = H * W;
    hipLaunchKernelGGL(scene_init_kernel, dim3((unsigned)B), block, 0, st, extrinsic, S, ws, stride, transform);
    hipLaunchKernelGGL(scene_conf_pass_kernel<0>, grid, block, 0, st, conf, (int)n, tile, conf_thres, ws, stride);
    hipLaunchKernelGGL(scene_conf_pass_kernel<1>, grid, block, 0, st, conf, (int)n, tile, conf_thres, ws, stride);
    hipLaunchKernelGGL(scene_conf_pass_kernel<2>, grid, block, 0, st, conf, (int)n, tile, conf_thres, ws, stride);
    hipLaunchKernelGGL(scene_conf_pass_kernel<3>, grid, block, 0, st, conf, (int)n, tile, conf_thres, ws, stride);
    hipLaunchKernelGGL(scene_mask_kernel, grid, block, 0, st, points, conf, images, (int)n, hw, tile, conf_thres, images_nchw ? 1 : 0,
                       mask_black_bg ? 1 : 0, mask_white_bg ? 1 : 0, ws, stride);
#define SKIMI_SCENE_XYZ(P)                                                                                                   \
    hipLaunchKernelGGL(scene_xyz_pass_kernel<P>, grid, block, 0, st, points, conf, images, (int)n, hw, tile, images_nchw ? 1 : 0, \
                       mask_black_bg ? 1 : 0, mask_white_bg ? 1 : 0, align ? 1 : 0, (long)cap, (const double*)transform, ws, stride, \
                       xyz, rgb)
    SKIMI_SCENE_XYZ(1);
    SKIMI_SCENE_XYZ(2);
    SKIMI_SCENE_XYZ(3);
#undef SKIMI_SCENE_XYZ
    hipLaunchKernelGGL(scene_finish_kernel, dim3((unsigned)B), block, 0, st, ws, stride, stats, (long long*)count);
    SKIMI_LAUNCH_CHECK();
    return SKIMI_OK;
}

}  // extern "C"
