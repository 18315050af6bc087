// The sampling half of the uint8 frame warps (lens.hip: undistort_u8_kernel, bev.hip: warp_perspective_u8_kernel): the
// two kernels differ only in how they get an output pixel's source position (su, sv).  Everything after that -- rule 7
// of the lens block in include/skimi.h: floor, the two weights, taps outside the source counting 0, the bilinear
// expression in its written order, floor(value + 0.5), the packing of a thread's kPix pixels into dwords and their
// store -- is here once, so the two warps round alike by construction.
//
// A thread owns kPix adjacent output pixels of one row: kPix * CH bytes, a whole number of dwords, which it packs in
// registers and writes as dwords when the output rows are dword-aligned (OW * CH % 4 == 0 and an aligned base), byte by
// byte otherwise and at a row's ragged end.  Block = kWarpX x kWarpY threads = 256 x 4 output pixels.
#pragma once
#include "common.h"

namespace skimi {

constexpr int kPix = 4, kWarpX = 64, kWarpY = 4;

// is the source position inside the frame's one-pixel margin?  false for a NaN
__device__ __forceinline__ bool warp_inside(double su, double sv, int H, int W) {
    return su > -1.0 && su < (double)W && sv > -1.0 && sv < (double)H;
}

// pixel p of the thread's span, sampled at (su, sv) (warp_inside holds) from src [H, W, CH], into its bytes of words
template <int CH>
__device__ __forceinline__ void warp_tap_pack(const unsigned char* __restrict__ src, int H, int W, double su, double sv, int p,
                                              unsigned int (&words)[CH]) {
    const double x0f = floor(su), y0f = floor(sv);
    const double a = su - x0f, b = sv - y0f;
    const int x0 = (int)x0f, y0 = (int)y0f;   // -1 .. W - 1, -1 .. H - 1
    const bool l = x0 >= 0, r = x0 + 1 < W, t = y0 >= 0, bt = y0 + 1 < H;
    const unsigned char* s00 = src + ((size_t)max(y0, 0) * W + max(x0, 0)) * CH;
    const size_t dx = (l && r) ? CH : 0, dy = (t && bt) ? (size_t)W * CH : 0;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        // every address lies inside the frame; a tap outside it counts 0
        const double p00 = (l && t) ? (double)s00[c] : 0.0;
        const double p01 = (r && t) ? (double)s00[(l ? dx : 0) + c] : 0.0;
        const double p10 = (l && bt) ? (double)s00[(t ? dy : 0) + c] : 0.0;
        const double p11 = (r && bt) ? (double)s00[(l ? dx : 0) + (t ? dy : 0) + c] : 0.0;
        const double val = (1.0 - b) * ((1.0 - a) * p00 + a * p01) + b * ((1.0 - a) * p10 + a * p11);
        const unsigned int q = (unsigned int)floor(val + 0.5);   // 0 .. 255
        const int byte = p * CH + c;
        words[byte >> 2] |= q << (8 * (byte & 3));
    }
}

// the thread's span from src = the address of pixel (u0, v): dwords where the rows allow it, else the bytes that exist
template <int CH>
__device__ __forceinline__ void span_load(const unsigned char* src, unsigned int (&words)[CH], int aligned, int u0, int W) {
    if (aligned && u0 + kPix <= W) {
        const unsigned int* dw = reinterpret_cast<const unsigned int*>(src);
#pragma unroll
        for (int w = 0; w < CH; ++w) words[w] = dw[w];
    } else {
        const int nb = min(kPix, W - u0) * CH;
#pragma unroll
        for (int w = 0; w < CH; ++w) words[w] = 0;
#pragma unroll
        for (int byte = 0; byte < kPix * CH; ++byte)
            if (byte < nb) words[byte >> 2] |= (unsigned int)src[byte] << (8 * (byte & 3));
    }
}

// the thread's span to dst = the address of output pixel (u0, v): dwords where the rows allow it, else the bytes that exist
template <int CH>
__device__ __forceinline__ void warp_store(unsigned char* __restrict__ dst, const unsigned int (&words)[CH], int aligned, int u0,
                                           int OW) {
    if (aligned && u0 + kPix <= OW) {
        unsigned int* dw = reinterpret_cast<unsigned int*>(dst);
#pragma unroll
        for (int w = 0; w < CH; ++w) dw[w] = words[w];
    } else {
        const int nb = min(kPix, OW - u0) * CH;
#pragma unroll
        for (int byte = 0; byte < kPix * CH; ++byte)
            if (byte < nb) dst[byte] = (unsigned char)(words[byte >> 2] >> (8 * (byte & 3)));
    }
}

}  // namespace skimi
