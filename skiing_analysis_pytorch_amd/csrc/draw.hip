// Drawing into uint8 frame clips (DESIGN §2 "Drawing"): an ordered list of discs, rings, capsules and 5 x 7 glyphs is
// composited into every frame of a clip in one launch.  The rules are in include/skimi.h; tests/draw_restated.py is the
// restatement.  Everything is integer (positions in 1/16 pixel, coverage 0 .. 16, opacity 0 .. 256), so the result is
// bitwise reproducible and bitwise the restatement's.
//
// A workgroup owns a block of 4 x 4 tiles of one frame (256 x 64 pixels), a tile is 64 x 16 pixels, and in a tile a thread
// owns kPix = 4 adjacent pixels of one row (warp_u8.h's span: whole dwords when the rows are dword-aligned, bytes otherwise
// and at a row's ragged end).  The shapes are tested twice, by the same conservative box test: the frame's list against the
// block, a shape a thread, and then the block's survivors against each tile; both times the indices that pass are written
// in list order into LDS (compact.h's ordered_rank).  Then every thread composites its pixels over the tile's list.  The
// shape index read back from LDS is the same in every lane and is made scalar, so the record's eight words arrive by
// scalar loads.  A pixel has one owner: no atomics.  A block or tile that no shape touches is copied, or left alone when
// out == frames.  Why two levels: on a 1080p clip with one skeleton 98 % of the tiles are empty, and with a workgroup a
// tile the test of 67 records cost more than the copy it guards (profiles/draw.md).
#include "common.h"
#include "compact.h"
#include "exact_int.h"
#include "raster_tiles.h"
#include "warp_u8.h"

namespace skimi {

namespace {

constexpr int kDrawThreads = kRasterThreads;

struct Shape {
    int kind, x0, y0, x1, y1, r, colour, opacity;
};

// a record as the rules read it: coordinates and radius saturated, opacity clamped, an unknown kind drawn as nothing
__device__ __forceinline__ Shape read_shape(const int* __restrict__ rec) {
    Shape s;
    s.kind = rec[0];
    s.x0 = sat20(rec[1]), s.y0 = sat20(rec[2]);
    s.x1 = rec[3], s.y1 = rec[4];
    s.r = sat20(rec[5]);
    s.colour = rec[6];
    s.opacity = min(max(rec[7], 0), 256);
    if (s.kind < SKIMI_DRAW_DISC || s.kind > SKIMI_DRAW_GLYPH) s.kind = SKIMI_DRAW_NONE;
    if (s.kind == SKIMI_DRAW_GLYPH) {
        s.r = max(s.r, 1);                                      // the scale
        s.x1 = (s.x1 >= 0x20 && s.x1 <= 0x7F) ? s.x1 : 0x7F;    // the character
    } else {
        s.x1 = sat20(s.x1), s.y1 = sat20(s.y1);
    }
    return s;
}

// can the shape change a pixel whose centre lies in [tx0, tx1] x [ty0, ty1] (1/16 pixel)?  Conservative: the shape's
// extent grown by its radius plus one pixel.
__device__ __forceinline__ bool touches(const Shape& s, int tx0, int ty0, int tx1, int ty1) {
    if (s.kind == SKIMI_DRAW_NONE || s.opacity == 0) return false;
    int bx0 = s.x0, by0 = s.y0, bx1 = s.x0, by1 = s.y0, g = 16;
    if (s.kind == SKIMI_DRAW_GLYPH) {
        bx0 = (s.x0 >> 4) * 16, by0 = (s.y0 >> 4) * 16;
        bx1 = bx0 + 16 * (5 * s.r - 1), by1 = by0 + 16 * (7 * s.r - 1);   // < 2^27
    } else if (s.kind == SKIMI_DRAW_RING) {
        g += s.r + s.x1;
    } else {
        g += s.r;
        if (s.kind == SKIMI_DRAW_CAPSULE) {
            bx0 = min(s.x0, s.x1), bx1 = max(s.x0, s.x1);
            by0 = min(s.y0, s.y1), by1 = max(s.y0, s.y1);
        }
    }
    return bx0 - g <= tx1 && bx1 + g >= tx0 && by0 - g <= ty1 && by1 + g >= ty0;
}

__device__ __forceinline__ int clamp16(int v) { return min(max(v, 0), 16); }

// coverage 0 .. 16 of the pixel whose centre is (16 u, 16 v); root: isqrt(|b - a|^2) of a capsule, font: [96, 7]
__device__ __forceinline__ int coverage(const Shape& s, double root, const unsigned char* __restrict__ font, int u, int v) {
    if (s.kind == SKIMI_DRAW_GLYPH) {
        const int cx = u - (s.x0 >> 4), cy = v - (s.y0 >> 4);
        if (cx < 0 || cy < 0 || cx >= 5 * s.r || cy >= 7 * s.r) return 0;
        const unsigned bits = font[(s.x1 - 0x20) * 7 + cy / s.r];
        return ((bits >> (cx / s.r)) & 1u) ? 16 : 0;
    }
    const double px = (double)(16 * u - s.x0), py = (double)(16 * v - s.y0);   // p - a
    double d;
    if (s.kind == SKIMI_DRAW_CAPSULE && root > 0.0) {
        const double ex = (double)(s.x1 - s.x0), ey = (double)(s.y1 - s.y0);   // b - a
        const double t = px * ex + py * ey, L2 = ex * ex + ey * ey;
        if (t <= 0.0) {
            d = isqrt_exact(px * px + py * py);
        } else if (t >= L2) {
            const double qx = px - ex, qy = py - ey;
            d = isqrt_exact(qx * qx + qy * qy);
        } else {
            d = floor_div_exact(fabs(px * ey - py * ex), root);
        }
    } else {
        d = isqrt_exact(px * px + py * py);
    }
    const int di = (int)d;   // <= 2^22 sqrt(2)
    if (s.kind == SKIMI_DRAW_RING) return clamp16(s.x1 + 8 - abs(di - s.r));
    return clamp16(s.r + 8 - di);
}

// `in` and `out` may be the same clip (in place): no __restrict__ on either
template <int CH>
__global__ __launch_bounds__(kDrawThreads) void draw_shapes_kernel(const unsigned char* in, unsigned char* out,
                                                                   const int* __restrict__ shapes, int shape_axes,
                                                                   const unsigned char* __restrict__ font, int F, int H, int W,
                                                                   int P, int aligned) {
    __shared__ unsigned short s_block[SKIMI_DRAW_MAX_SHAPES], s_list[SKIMI_DRAW_MAX_SHAPES];
    __shared__ unsigned s_wtot[2][kDrawThreads / 64];
    const int tid = threadIdx.x;
    const int img = blockIdx.z;
    const int list = shape_axes == 2 ? 0 : shape_axes == 3 ? img % F : img;
    const int* __restrict__ recs = shapes + (size_t)list * P * 8;
    const int bx0 = blockIdx.x * kBlockW, by0 = blockIdx.y * kBlockH;   // inside the frame
    const size_t frame = (size_t)img * H * W * CH;
    const bool in_place = in == out;

    // the block's list, in list order: a shape a thread, a round of kDrawThreads shapes at a time
    unsigned nb = 0;
    int buf = 0;
    {
        const int x1 = 16 * (min(bx0 + kBlockW, W) - 1), y1 = 16 * (min(by0 + kBlockH, H) - 1);
        for (int i0 = 0; i0 < P; i0 += kDrawThreads) {   // uniform trip count: every thread reaches the barrier
            const int i = i0 + tid;
            const bool kept = i < P && touches(read_shape(recs + (size_t)i * 8), 16 * bx0, 16 * by0, x1, y1);
            list_round(kept, i, s_block, nb, s_wtot, buf);
        }
    }
    if (nb == 0) {                 // workgroup-uniform: nothing to draw on the whole block
        if (in_place) return;
        // the copy, a wave a row of the block (kBlockW * CH contiguous bytes), four rows in flight a thread
        const int u0 = bx0 + (tid & 63) * kPix;
        if (u0 >= W) return;
        constexpr int kRows = kDrawThreads / 64, kFly = 4;
        for (int r0 = tid >> 6; r0 < kBlockH; r0 += kRows * kFly) {
            unsigned int words[kFly][CH];
#pragma unroll
            for (int k = 0; k < kFly; ++k) {
                const int v = by0 + r0 + k * kRows;
                if (v < H) span_load<CH>(in + frame + ((size_t)v * W + u0) * CH, words[k], aligned, u0, W);
            }
#pragma unroll
            for (int k = 0; k < kFly; ++k) {
                const int v = by0 + r0 + k * kRows;
                if (v < H) warp_store<CH>(out + frame + ((size_t)v * W + u0) * CH, words[k], aligned, u0, W);
            }
        }
        return;
    }
    __syncthreads();               // s_block

    constexpr int kCol = CH == 4 ? 3 : CH;   // channel 3 of a 4-channel frame is never written
    for (int t = 0; t < kTilesX * kTilesY; ++t) {   // the block's tiles; everything that skips one is workgroup-uniform
        const int px0 = bx0 + (t % kTilesX) * kTileW, py0 = by0 + (t / kTilesX) * kTileH;
        if (px0 >= W || py0 >= H) continue;
        const int tx1 = 16 * (min(px0 + kTileW, W) - 1), ty1 = 16 * (min(py0 + kTileH, H) - 1);
        // the tile's list out of the block's, order kept.  The barrier inside the first round is also what keeps this
        // tile's writes to s_list behind every thread's reads of the tile before (nb > 0: there is a first round).
        unsigned n = 0;
        for (unsigned i0 = 0; i0 < nb; i0 += kDrawThreads) {
            const unsigned i = i0 + tid;
            const int idx = i < nb ? (int)s_block[i] : 0;
            const bool kept = i < nb && touches(read_shape(recs + (size_t)idx * 8), 16 * px0, 16 * py0, tx1, ty1);
            list_round(kept, idx, s_list, n, s_wtot, buf);
        }
        if (n == 0 && in_place) continue;
        __syncthreads();           // s_list

        const int v = py0 + tid / kSpanX;
        const int u0 = px0 + (tid % kSpanX) * kPix;
        if (v >= H || u0 >= W) continue;   // this thread owns no pixel of the tile; it still takes part in the next tile's barriers
        const size_t at = frame + ((size_t)v * W + u0) * CH;
        unsigned int words[CH];
        span_load<CH>(in + at, words, aligned, u0, W);
        for (unsigned k = 0; k < n; ++k) {
            const int idx = __builtin_amdgcn_readfirstlane((int)s_list[k]);   // the same in every lane: scalar record loads
            const Shape s = read_shape(recs + (size_t)idx * 8);
            if (!touches(s, 16 * u0, 16 * v, 16 * (u0 + kPix - 1), 16 * v)) continue;   // not on this thread's span
            double root = 0.0;
            if (s.kind == SKIMI_DRAW_CAPSULE) {
                const double ex = (double)(s.x1 - s.x0), ey = (double)(s.y1 - s.y0);
                root = isqrt_exact(ex * ex + ey * ey);   // 0 iff a = b: the disc
            }
#pragma unroll
            for (int p = 0; p < kPix; ++p) {
                if (u0 + p >= W) continue;
                const int a = coverage(s, root, font, u0 + p, v) * s.opacity;   // 0 .. 4096
                if (a == 0) continue;
#pragma unroll
                for (int c = 0; c < kCol; ++c) {
                    const int byte = p * CH + c, sh = 8 * (byte & 3);
                    const int cur = (int)((words[byte >> 2] >> sh) & 255u);
                    const int col = (s.colour >> (8 * c)) & 255;
                    const unsigned int q = (unsigned int)((cur * (4096 - a) + col * a + 2048) >> 12);   // 0 .. 255
                    words[byte >> 2] = (words[byte >> 2] & ~(255u << sh)) | (q << sh);
                }
            }
        }
        warp_store<CH>(out + at, words, aligned, u0, W);
    }
}

}  // namespace

}  // namespace skimi

using namespace skimi;

extern "C" {

int skimi_draw_shapes_u8(const uint8_t* frames, uint8_t* out, const int32_t* shapes, int32_t shape_axes, const uint8_t* font,
                         int32_t C, int32_t F, int32_t H, int32_t W, int32_t ch, int32_t P, void* stream) {
    SKIMI_CHECK_ARG(ch == 1 || ch == 3 || ch == 4, "skimi_draw_shapes_u8: %d channels (1, 3 or 4)", ch);
    SKIMI_CHECK_ARG(C >= 1 && F >= 1 && (int64_t)C * F <= 65535, "skimi_draw_shapes_u8: C = %d, F = %d outside 1 <= C, F, C * F <= 65535",
                    C, F);
    SKIMI_CHECK_ARG(H >= 1 && W >= 1 && H <= SKIMI_LENS_MAX_SIDE && W <= SKIMI_LENS_MAX_SIDE,
                    "skimi_draw_shapes_u8: frame %d x %d outside 1 .. %d a side", W, H, SKIMI_LENS_MAX_SIDE);
    SKIMI_CHECK_ARG(P >= 0 && P <= SKIMI_DRAW_MAX_SHAPES, "skimi_draw_shapes_u8: P = %d outside 0 .. %d", P, SKIMI_DRAW_MAX_SHAPES);
    SKIMI_CHECK_ARG(shape_axes >= 2 && shape_axes <= 4, "skimi_draw_shapes_u8: shape_axes = %d (2: [P, 8], 3: [F, P, 8], 4: [C, F, P, 8])",
                    shape_axes);
    SKIMI_CHECK_ARG(frames && out && font && (shapes || P == 0), "skimi_draw_shapes_u8: NULL frames, output, shapes or font");
    if (P == 0 && frames == out) return SKIMI_OK;
    const int aligned = ((int64_t)W * ch) % 4 == 0 && ((uintptr_t)frames & 3) == 0 && ((uintptr_t)out & 3) == 0;
    const dim3 grid((unsigned)cdiv(W, kBlockW), (unsigned)cdiv(H, kBlockH), (unsigned)(C * F)), block(kDrawThreads);
    if (ch == 1)
        hipLaunchKernelGGL(draw_shapes_kernel<1>, grid, block, 0, (hipStream_t)stream, frames, out, shapes, shape_axes, font, F, H, W, P,
                           aligned);
    else if (ch == 3)
        hipLaunchKernelGGL(draw_shapes_kernel<3>, grid, block, 0, (hipStream_t)stream, frames, out, shapes, shape_axes, font, F, H, W, P,
                           aligned);
    else
        hipLaunchKernelGGL(draw_shapes_kernel<4>, grid, block, 0, (hipStream_t)stream, frames, out, shapes, shape_axes, font, F, H, W, P,
                           aligned);
    SKIMI_LAUNCH_CHECK();
    return SKIMI_OK;
}

}  // extern "C"
