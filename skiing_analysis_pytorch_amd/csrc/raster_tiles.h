// The tiling and the ordered list rounds that the two rasterisers share (draw.hip: draw_shapes_kernel, scene_view.hip:
// scene_resolve_kernel).  A workgroup of kRasterThreads owns a block of kTilesX x kTilesY tiles of one frame (256 x 64
// pixels), a tile is 64 x 16 pixels, and in a tile a thread owns kPix adjacent pixels of one row (warp_u8.h's span).  The
// record list is tested twice, against the block and then the block's survivors against each tile; both times the indices
// that pass go in list order into LDS through list_round.  The records and their box tests differ between the two kernels
// and stay with them; the barrier and buffer contract is here once.
#pragma once
#include "common.h"
#include "compact.h"
#include "warp_u8.h"

namespace skimi {

constexpr int kRasterThreads = 256;
constexpr int kTileW = 64, kTileH = 16;           // kTileW / kPix * kTileH = kRasterThreads
constexpr int kSpanX = kTileW / kPix;             // threads along a tile row
constexpr int kTilesX = 4, kTilesY = 4;           // a workgroup's block of tiles
constexpr int kBlockW = kTileW * kTilesX, kBlockH = kTileH * kTilesY;
static_assert(kBlockW == 64 * kPix, "a wave a row of the block");
static_assert(kSpanX * kTileH == kRasterThreads, "a thread a span");

// One round of the ordered compaction: the calling thread's candidate `idx` (kept or not); the kept ones go to dst in
// candidate order behind the n already there (the caller's lists hold every index that can be kept).  Every thread of the
// workgroup calls it (ordered_rank's contract: one barrier inside); buf alternates over ALL calls of the kernel, block list
// and tile lists alike.
__device__ __forceinline__ void list_round(bool kept, int idx, unsigned short* dst, unsigned& n, unsigned (*s_wtot)[kRasterThreads / 64],
                                           int& buf) {
    unsigned chunk;
    const unsigned rank = ordered_rank<kRasterThreads / 64>(kept, s_wtot[buf], chunk);
    if (kept) dst[n + rank] = (unsigned short)idx;
    n += chunk;
    buf ^= 1;
}

}  // namespace skimi
