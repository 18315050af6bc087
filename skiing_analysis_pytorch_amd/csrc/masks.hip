// Mask analysis (DESIGN §2 "Masks"): connected components, the exact Euclidean distance transform and its argmax, boxes,
// pairwise IoU on bit-packed masks, and greedy NMS on an IoU matrix.  The rules are in include/skimi.h;
// tests/masks_restated.py is the restatement.  Everything is integer (the two floats, dist and iou, are one stated operation
// on integers), every sum is an integer atomic or a fixed loop, and every extremum is unique, so the results are bitwise
// reproducible, bitwise the restatement's, and the same for a mask alone as inside a batch.  Nothing is read back and the
// number of launches is fixed by the shapes: no kernel is relaunched until "nothing changed".
//
// Components are a block union-find.  The parent of a foreground pixel is a pixel of its component with a linear index
// that is not larger (itself: a root), background is -1.  cc_tile labels a 64 x 16 tile in LDS, cc_seams joins the pairs of
// neighbours that a tile border separates with atomicMin on the global array, and the root of a component is then its
// SMALLEST linear index, which is also its first pixel in raster order: unique, whatever order the waves ran in.  The roots
// are numbered in raster order by compact.h's ordered count / offset pair, and areas and stats are summed a tile at a time in
// LDS before one global atomic a (tile, group) pair.
#include "common.h"
#include "compact.h"

namespace skimi {

namespace {

constexpr int kT = 256;
constexpr int kTileW = 64, kTileH = 16, kTilePix = kTileW * kTileH;
constexpr int kChunk = 4096;          // pixels of a mask a workgroup numbers the roots of
constexpr int kMinBias = 1 << 20;     // a minimum m is summed as the maximum of kMinBias - m: zero stays "nothing yet"
constexpr int kEdtInf = 1 << 15;      // the vertical distance of a column without a zero: kEdtInf^2 = SKIMI_EDT_NONE
static_assert(kEdtInf * kEdtInf == SKIMI_EDT_NONE, "a column without a zero squares to SKIMI_EDT_NONE");
static_assert(kMinBias > SKIMI_MASK_MAX_SIDE, "kMinBias - coordinate stays positive");

constexpr int kWg = __HIP_MEMORY_SCOPE_WORKGROUP, kAgent = __HIP_MEMORY_SCOPE_AGENT;

// a parent as the other threads' atomics leave it: a relaxed atomic load (LDS: workgroup scope; global memory inside the
// launch that merges: agent scope, past the caches that another CU's atomics do not refresh)
template <int kScope>
__device__ __forceinline__ int parent_of(const int* L, int x) {
    return __hip_atomic_load(L + x, __ATOMIC_RELAXED, kScope);
}

// The root above x.  Terminates by construction: L[x] <= x for every foreground x at every time (it starts as x and only
// atomicMin, with a smaller foreground index, ever writes it), so each step strictly decreases x, at most x steps.
template <int kScope>
__device__ __forceinline__ int find_root(const int* L, int x) {
    for (int v = parent_of<kScope>(L, x); v != x; v = parent_of<kScope>(L, x)) x = v;
    return x;
}

// Join the sets of a and b.  The larger root is hung under the smaller by atomicMin, which returns what was there: if that
// is still the root itself the link is made; if not, another thread got there first, the entry now holds min(theirs, ours)
// and what it held (`old`, smaller than b, of b's set) is joined with a instead.  Terminates by construction: no thread
// waits for another, and a round is repeated only when some other thread LOWERED an entry between this thread's find and
// its atomicMin; entries only ever decrease and are bounded below by 0, so there are finitely many such rounds in all.
template <int kScope>
__device__ __forceinline__ void unite(int* L, int a, int b) {
    for (;;) {
        a = find_root<kScope>(L, a);
        b = find_root<kScope>(L, b);
        if (a == b) return;
        if (a > b) {
            const int t = a;
            a = b, b = t;
        }
        const int old = atomicMin(&L[b], a);
        if (old == b) return;
        b = old;
    }
}

struct Tile {
    int b, x0, y0;
};
__device__ __forceinline__ Tile tile_of(int tilesX, int tilesY) {
    const long blk = blockIdx.x;
    Tile t;
    t.x0 = (int)(blk % tilesX) * kTileW;
    t.y0 = (int)((blk / tilesX) % tilesY) * kTileH;
    t.b = (int)(blk / ((long)tilesX * tilesY));
    return t;
}

// ---- components ------------------------------------------------------------------------------------------------------------
// Label one tile in LDS and store every pixel's tile root as its parent.  Local indices ly * 64 + lx order the tile's pixels
// as the image's linear indices do, so the smallest local index is the smallest linear index.
__global__ __launch_bounds__(kT) void cc_tile_kernel(const unsigned char* __restrict__ masks, int* __restrict__ parent, int H, int W,
                                                     int tilesX, int tilesY, int conn8) {
    __shared__ int s_par[kTilePix];
    const Tile t = tile_of(tilesX, tilesY);
    const size_t img = (size_t)t.b * H * W;
    const int tid = threadIdx.x;
    for (int l = tid; l < kTilePix; l += kT) {
        const int x = t.x0 + (l & 63), y = t.y0 + (l >> 6);
        s_par[l] = (x < W && y < H && masks[img + (size_t)y * W + x]) ? l : -1;
    }
    __syncthreads();
    // s_par[n] >= 0 iff n is foreground, at every time.  Every pixel is joined with its neighbours behind it: left and up, and
    // for 8 up-left and up-right, which are already joined with `up` (their horizontal neighbour) where that is foreground.
    for (int l = tid; l < kTilePix; l += kT) {
        if (parent_of<kWg>(s_par, l) < 0) continue;
        const int lx = l & 63, ly = l >> 6;
        if (lx > 0 && parent_of<kWg>(s_par, l - 1) >= 0) unite<kWg>(s_par, l, l - 1);
        if (ly == 0) continue;
        if (parent_of<kWg>(s_par, l - 64) >= 0) {
            unite<kWg>(s_par, l, l - 64);
        } else if (conn8) {
            if (lx > 0 && parent_of<kWg>(s_par, l - 65) >= 0) unite<kWg>(s_par, l, l - 65);
            if (lx < 63 && parent_of<kWg>(s_par, l - 63) >= 0) unite<kWg>(s_par, l, l - 63);
        }
    }
    __syncthreads();
    for (int l = tid; l < kTilePix; l += kT) {
        const int x = t.x0 + (l & 63), y = t.y0 + (l >> 6);
        if (x >= W || y >= H) continue;
        int v = -1;
        if (s_par[l] >= 0) {
            const int r = find_root<kWg>(s_par, l);
            v = (t.y0 + (r >> 6)) * W + t.x0 + (r & 63);
        }
        parent[img + (size_t)y * W + x] = v;
    }
}

// Join across the tile borders.  An item is a pixel of the first row of a tile row (the first (tilesY - 1) W items) or of
// the first column of a tile column ((tilesX - 1) H items); it is joined with its neighbours on the other side.  Every pair
// of neighbours in different tiles is met once: a pair across a horizontal border from the lower pixel, a pair across a
// vertical border only from the pixel right of it, and there the diagonal that also crosses a horizontal border is left to
// that border's item.
__global__ __launch_bounds__(kT) void cc_seams_kernel(int* __restrict__ parent, int H, int W, int tilesX, int tilesY, int conn8,
                                                      int groups) {
    const int b = blockIdx.x / groups;
    const long item = (long)(blockIdx.x % groups) * kT + threadIdx.x;
    const long nH = (long)(tilesY - 1) * W, nV = (long)(tilesX - 1) * H;
    if (item >= nH + nV) return;
    int* L = parent + (size_t)b * H * W;
    auto fg = [&](int x, int y) { return parent_of<kAgent>(L, y * W + x) >= 0; };
    if (item < nH) {
        const int x = (int)(item % W), y = (int)(item / W + 1) * kTileH, p = y * W + x;   // 1 <= y < H
        if (!fg(x, y)) return;
        if (fg(x, y - 1)) unite<kAgent>(L, p, p - W);
        if (conn8 && x > 0 && fg(x - 1, y - 1)) unite<kAgent>(L, p, p - W - 1);
        if (conn8 && x + 1 < W && fg(x + 1, y - 1)) unite<kAgent>(L, p, p - W + 1);
    } else {
        const long it = item - nH;
        const int y = (int)(it % H), x = (int)(it / H + 1) * kTileW, p = y * W + x;       // 1 <= x < W
        if (!fg(x, y)) return;
        if (fg(x - 1, y)) unite<kAgent>(L, p, p - 1);
        if (conn8 && y % kTileH != 0 && fg(x - 1, y - 1)) unite<kAgent>(L, p, p - W - 1);
        if (conn8 && y + 1 < H && (y + 1) % kTileH != 0 && fg(x - 1, y + 1)) unite<kAgent>(L, p, p + W - 1);
    }
}

// The group of a tile's pixel in the tile sums: its parent where that lies in the same tile, else itself.  A group is part of
// one component (a pixel and its parent always are), and its key is one of its own pixels.
__device__ __forceinline__ int group_key(const Tile& t, int W, int l, int v) {
    if (v < 0) return l;
    const int vy = v / W, vx = v - vy * W;
    const bool in = vx >= t.x0 && vx < t.x0 + kTileW && vy >= t.y0 && vy < t.y0 + kTileH;
    return in ? (vy - t.y0) * 64 + vx - t.x0 : l;
}

// Areas: count a tile's pixels by group in LDS, then one atomic a group onto the component's root in `areas` (zeroed).
// parent is only read in this launch: plain loads.
__global__ __launch_bounds__(kT) void cc_area_kernel(const int* __restrict__ parent, int* __restrict__ areas, int H, int W, int tilesX,
                                                     int tilesY) {
    __shared__ int s_cnt[kTilePix];
    const Tile t = tile_of(tilesX, tilesY);
    const int* L = parent + (size_t)t.b * H * W;
    const int tid = threadIdx.x;
    for (int l = tid; l < kTilePix; l += kT) s_cnt[l] = 0;
    __syncthreads();
    for (int l = tid; l < kTilePix; l += kT) {
        const int x = t.x0 + (l & 63), y = t.y0 + (l >> 6);
        if (x >= W || y >= H) continue;
        const int v = L[y * W + x];
        if (v >= 0) atomicAdd(&s_cnt[group_key(t, W, l, v)], 1);
    }
    __syncthreads();
    for (int l = tid; l < kTilePix; l += kT) {
        const int c = s_cnt[l];
        if (c == 0) continue;   // c > 0: l is a foreground pixel of the image
        int x = (t.y0 + (l >> 6)) * W + t.x0 + (l & 63);
        for (int v = L[x]; v != x; v = L[x]) x = v;   // find_root's loop on a parent array at rest
        atomicAdd(&areas[(size_t)t.b * H * W + x], c);
    }
}

// The dense numbering: "is this pixel a root" through compact.h's ordered count / offset pair, a mask a stream of `groups`
// chunks.  The write launch leaves label k (1-based, raster order of the roots) in the root's own parent entry as -1 - k.
__global__ __launch_bounds__(kT) void cc_root_count_kernel(const int* __restrict__ parent, unsigned* __restrict__ bc, int HW, int groups) {
    __shared__ unsigned s_cnt;
    const int b = blockIdx.x / groups, g = blockIdx.x % groups;
    const int* L = parent + (size_t)b * HW;
    const long beg = (long)g * kChunk, end = beg + kChunk < HW ? beg + kChunk : (long)HW;
    const unsigned n = tile_count<kT>(beg, end, s_cnt, [&](long i) { return L[i] == (int)i; });
    if (threadIdx.x == 0) bc[blockIdx.x] = n;
}

__global__ __launch_bounds__(kT) void cc_root_number_kernel(int* __restrict__ parent, const unsigned* __restrict__ bc,
                                                            int* __restrict__ count, int HW, int groups) {
    __shared__ unsigned s_total, s_offset;
    __shared__ unsigned s_wtot[2][kT / 64];
    const int b = blockIdx.x / groups, g = blockIdx.x % groups;
    int* L = parent + (size_t)b * HW;
    group_offsets<kT>(bc + (size_t)b * groups, groups, g, s_total, s_offset);
    if (g == 0 && threadIdx.x == 0) count[b] = (int)s_total;
    const long beg = (long)g * kChunk, end = beg + kChunk < HW ? beg + kChunk : (long)HW;
    // a thread tests and rewrites only its own entry, inside its own chunk
    ordered_write<kT>(beg, end, (long)s_offset, s_wtot, [&](long i) { return L[i] == (int)i; }, [&](long i, long row) { L[i] = -2 - (int)row; });
}

// Labels, areas and the stats table.  A root's parent entry is now -1 - label and every other foreground entry is a smaller
// foreground index, so the walk strictly decreases until it meets a negative entry.  areas holds a component's area at its
// root; the other pixels copy it (a root is never written here).  Stats are summed by group in LDS (minima as maxima of
// kMinBias - m), then one set of 64-bit atomics a group into the zeroed table.
template <bool kStats>
__global__ __launch_bounds__(kT) void cc_label_kernel(const int* __restrict__ parent, int* __restrict__ labels, int* areas,
                                                      unsigned long long* __restrict__ stats, int H, int W, int tilesX, int tilesY,
                                                      int maxc) {
    __shared__ int s_tab[kStats ? 8 : 1][kStats ? kTilePix : 1];   // area, x_min', y_min', x_max, y_max, sum x, sum y, label
    const Tile t = tile_of(tilesX, tilesY);
    const size_t img = (size_t)t.b * H * W;
    const int* L = parent + img;
    const int tid = threadIdx.x;
    if constexpr (kStats) {
        for (int l = tid; l < kTilePix; l += kT)
#pragma unroll
            for (int k = 0; k < 8; ++k) s_tab[k][l] = 0;
        __syncthreads();
    }
    for (int l = tid; l < kTilePix; l += kT) {
        const int x = t.x0 + (l & 63), y = t.y0 + (l >> 6);
        if (x >= W || y >= H) continue;
        const int p = y * W + x, v0 = L[p];
        if (v0 == -1) {
            labels[img + p] = 0;
            continue;
        }
        int root = p, v = v0;
        while (v >= 0) {
            root = v;
            v = L[root];
        }
        const int label = -1 - v;
        labels[img + p] = label;
        if (root != p) areas[img + p] = areas[img + root];
        if constexpr (kStats) {
            s_tab[7][l] = label;
            if (label <= maxc) {
                const int k = group_key(t, W, l, v0);
                atomicAdd(&s_tab[0][k], 1);
                atomicMax(&s_tab[1][k], kMinBias - x);
                atomicMax(&s_tab[2][k], kMinBias - y);
                atomicMax(&s_tab[3][k], x);
                atomicMax(&s_tab[4][k], y);
                atomicAdd(&s_tab[5][k], x);   // <= 1024 * 4095
                atomicAdd(&s_tab[6][k], y);
            }
        }
    }
    if constexpr (kStats) {
        __syncthreads();
        for (int l = tid; l < kTilePix; l += kT) {
            if (s_tab[0][l] == 0) continue;   // else l is a foreground pixel whose label is in the table
            unsigned long long* row = stats + ((size_t)t.b * maxc + (s_tab[7][l] - 1)) * 7;
            atomicAdd(row + 0, (unsigned long long)s_tab[0][l]);
            atomicMax(row + 1, (unsigned long long)s_tab[1][l]);
            atomicMax(row + 2, (unsigned long long)s_tab[2][l]);
            atomicMax(row + 3, (unsigned long long)s_tab[3][l]);
            atomicMax(row + 4, (unsigned long long)s_tab[4][l]);
            atomicAdd(row + 5, (unsigned long long)s_tab[5][l]);
            atomicAdd(row + 6, (unsigned long long)s_tab[6][l]);
        }
    }
}

// the minima back from their biased form; a row without a component stays zero
__global__ __launch_bounds__(kT) void cc_stats_finish_kernel(long long* __restrict__ stats, long rows) {
    const long r = (long)blockIdx.x * kT + threadIdx.x;
    if (r >= rows || stats[r * 7] == 0) return;
    stats[r * 7 + 1] = kMinBias - stats[r * 7 + 1];
    stats[r * 7 + 2] = kMinBias - stats[r * 7 + 2];
}

// ---- distance transform ----------------------------------------------------------------------------------------------------
// Column pass, a thread a column, coalesced across x: g = the distance to the nearest zero of the column, down and then up;
// outside the image is a zero (border) or nothing (kEdtInf, which saturates).
__global__ __launch_bounds__(kT) void edt_columns_kernel(const unsigned char* __restrict__ masks, int* __restrict__ g, int H, int W,
                                                         int groups, int border) {
    const int b = blockIdx.x / groups, x = (blockIdx.x % groups) * kT + threadIdx.x;
    if (x >= W) return;
    const unsigned char* m = masks + (size_t)b * H * W + x;
    int* col = g + (size_t)b * H * W + x;
    int d = border ? 0 : kEdtInf;
    for (int y = 0; y < H; ++y) {
        d = m[(size_t)y * W] ? min(d + 1, kEdtInf) : 0;
        col[(size_t)y * W] = d;
    }
    d = border ? 0 : kEdtInf;
    for (int y = H - 1; y >= 0; --y) {
        const int v = col[(size_t)y * W];
        d = v == 0 ? 0 : min(d + 1, kEdtInf);
        col[(size_t)y * W] = min(v, d);
    }
}

// Row pass, a workgroup a row, in place: the row's g^2 goes to LDS, then every pixel minimises r^2 + g^2(x +- r) over r.  No
// candidate at distance r is below r^2 + the row's smallest g^2, so the widening stops there; r grows by one a round and
// ends at the row's far end at the latest.  Sums stay below 2^30 + 2^24.
__global__ __launch_bounds__(kT) void edt_rows_kernel(int* __restrict__ d2, float* __restrict__ dist, int W, int border) {
    __shared__ int s_g2[SKIMI_MASK_MAX_SIDE];
    __shared__ int s_min;
    const int tid = threadIdx.x;
    int* row = d2 + (size_t)blockIdx.x * W;
    if (tid == 0) s_min = SKIMI_EDT_NONE;
    __syncthreads();
    int mn = SKIMI_EDT_NONE;
    for (int x = tid; x < W; x += kT) {
        const int gx = row[x];
        s_g2[x] = gx * gx;
        mn = min(mn, gx * gx);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mn = min(mn, __shfl_xor(mn, o, 64));
    if ((tid & 63) == 0) atomicMin(&s_min, mn);
    __syncthreads();
    const int floor2 = s_min;
    for (int x = tid; x < W; x += kT) {
        int best = s_g2[x];
        if (border) best = min(best, min((x + 1) * (x + 1), (W - x) * (W - x)));
        const int far = max(x, W - 1 - x);
        for (int r = 1; r <= far; ++r) {
            const int r2 = r * r;
            if (r2 + floor2 >= best) break;
            if (x - r >= 0) best = min(best, r2 + s_g2[x - r]);
            if (x + r < W) best = min(best, r2 + s_g2[x + r]);
        }
        row[x] = best;
        if (dist) dist[(size_t)blockIdx.x * W + x] = best >= SKIMI_EDT_NONE ? __builtin_inff() : (float)sqrt((double)best);
    }
}

// The pixel of largest d2, ties to the first in raster order: the maximum of the key (d2 high, inverted index low), which is
// unique, so the order of the reduction cannot matter.
__global__ __launch_bounds__(1024) void argmax_kernel(const int* __restrict__ d2, int* __restrict__ xy, int* __restrict__ best, int HW,
                                                      int W) {
    __shared__ unsigned long long s_key[16];
    const int* v = d2 + (size_t)blockIdx.x * HW;
    unsigned long long key = 0;
    for (int i = threadIdx.x; i < HW; i += 1024) {
        const unsigned long long k = ((unsigned long long)(unsigned)v[i] << 32) | (0xFFFFFFFFu - (unsigned)i);
        key = k > key ? k : key;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long k = __shfl_xor(key, o, 64);
        key = k > key ? k : key;
    }
    if ((threadIdx.x & 63) == 0) s_key[threadIdx.x >> 6] = key;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 16; ++w) key = s_key[w] > key ? s_key[w] : key;
        const int i = (int)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull));
        xy[2 * (size_t)blockIdx.x] = i % W;
        xy[2 * (size_t)blockIdx.x + 1] = i / W;
        best[blockIdx.x] = (int)(key >> 32);
    }
}

// ---- packed masks: boxes and IoU -------------------------------------------------------------------------------------------
// The one packing: bit i of word k of a mask is pixel 64 k + i of the flattened mask, zero behind its end.  A wave packs the
// eight words k0 .. k0 + 7: eight byte loads a lane in flight, eight ballots; lane j < 8 returns word k0 + j.
__device__ __forceinline__ unsigned long long pack_words8(const unsigned char* __restrict__ mask, long HW, long k0) {
    const int lane = threadIdx.x & 63;
    unsigned char v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const long pixel = (k0 + j) * 64 + lane;
        v[j] = pixel < HW ? mask[pixel] : (unsigned char)0;
    }
    unsigned long long mine = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const unsigned long long w = __ballot(v[j] != 0);
        if (lane == j) mine = w;
    }
    return mine;
}

constexpr int kPackWords = (kT / 64) * 8;   // words a workgroup packs
__global__ __launch_bounds__(kT) void pack_kernel(const unsigned char* __restrict__ masks, unsigned long long* __restrict__ words, long HW,
                                                  long nw, int groups) {
    const long b = blockIdx.x / groups;
    const long k0 = (long)(blockIdx.x % groups) * kPackWords + (threadIdx.x >> 6) * 8;   // wave-uniform
    const unsigned long long w = pack_words8(masks + b * HW, HW, k0);
    const int lane = threadIdx.x & 63;
    if (lane < 8 && k0 + lane < nw) words[b * nw + k0 + lane] = w;
}

// A workgroup a mask.  A word is cut into the pieces that lie in one row; the lowest and highest bit of a piece are columns.
__global__ __launch_bounds__(1024) void boxes_kernel(const unsigned long long* __restrict__ words, int* __restrict__ xyxy,
                                                   int* __restrict__ area, int H, int W, long nw) {
    __shared__ int s_box[5];
    const int tid = threadIdx.x;
    if (tid == 0) s_box[0] = W, s_box[1] = H, s_box[2] = 0, s_box[3] = 0, s_box[4] = 0;
    __syncthreads();
    int x0 = W, y0 = H, x1 = 0, y1 = 0, n = 0;
    const unsigned long long* wd = words + (size_t)blockIdx.x * nw;
    for (long k = tid; k < nw; k += blockDim.x) {
        unsigned long long w = wd[k];
        n += __popcll(w);
        const int base = (int)(k * 64);
        while (w) {   // every round clears at least the lowest set bit
            const int lo = __builtin_ctzll(w), idx = base + lo, y = idx / W;
            const int row_end = (y + 1) * W - base;   // > lo: the bit behind the row's last pixel
            const unsigned long long piece = row_end >= 64 ? w : w & ((1ull << row_end) - 1ull);
            const int hi = 63 - __builtin_clzll(piece), xl = idx - y * W;
            x0 = min(x0, xl), x1 = max(x1, xl + hi - lo), y0 = min(y0, y), y1 = max(y1, y);
            w &= ~piece;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        x0 = min(x0, __shfl_xor(x0, o, 64)), y0 = min(y0, __shfl_xor(y0, o, 64));
        x1 = max(x1, __shfl_xor(x1, o, 64)), y1 = max(y1, __shfl_xor(y1, o, 64));
        n += __shfl_xor(n, o, 64);
    }
    if ((tid & 63) == 0) {
        atomicMin(&s_box[0], x0), atomicMin(&s_box[1], y0), atomicMax(&s_box[2], x1), atomicMax(&s_box[3], y1);
        atomicAdd(&s_box[4], n);
    }
    __syncthreads();
    if (tid < 4) xyxy[4 * (size_t)blockIdx.x + tid] = s_box[tid];
    if (tid == 4) area[blockIdx.x] = s_box[4];
}

// A workgroup a 16 x 16 tile of pairs, a thread a pair, over all the words: 64 words of the 16 + 16 masks at a time in LDS
// (rows padded by a word: the 16 b rows a wave reads lie on different banks), so a staged word serves 16 pairs.
constexpr int kPairs = 16, kWordsLds = 64;
__global__ __launch_bounds__(kT) void iou_kernel(const unsigned long long* __restrict__ a, const unsigned long long* __restrict__ b,
                                                 float* __restrict__ iou, int* __restrict__ inter, int* __restrict__ uni, int N, int M,
                                                 long nw) {
    __shared__ unsigned long long s_a[kPairs][kWordsLds + 1], s_b[kPairs][kWordsLds + 1];
    const int tid = threadIdx.x, i = tid / kPairs, j = tid % kPairs;
    const int n0 = blockIdx.y * kPairs, m0 = blockIdx.x * kPairs;
    const size_t clip = blockIdx.z;
    int ni = 0, nu = 0;
    for (long k0 = 0; k0 < nw; k0 += kWordsLds) {   // uniform trip count
        for (int e = tid; e < kPairs * kWordsLds; e += kT) {
            const int r = e / kWordsLds, c = e % kWordsLds;
            const bool in = k0 + c < nw;
            s_a[r][c] = (in && n0 + r < N) ? a[(clip * N + n0 + r) * nw + k0 + c] : 0ull;
            s_b[r][c] = (in && m0 + r < M) ? b[(clip * M + m0 + r) * nw + k0 + c] : 0ull;
        }
        __syncthreads();
#pragma unroll 8
        for (int c = 0; c < kWordsLds; ++c) {
            const unsigned long long wa = s_a[i][c], wb = s_b[j][c];
            ni += __popcll(wa & wb);
            nu += __popcll(wa | wb);
        }
        __syncthreads();
    }
    if (n0 + i < N && m0 + j < M) {
        const size_t at = (clip * N + n0 + i) * M + m0 + j;
        inter[at] = ni;
        uni[at] = nu;
        iou[at] = (float)ni / (float)max(nu, 1);
    }
}

// ---- greedy NMS ------------------------------------------------------------------------------------------------------------
// A workgroup a problem.  The order is the descending order of exact keys (the score's bits made monotone, then the inverted
// index: unique, ties to the lower index), found by counting.  Then 64 places of the order at a time: the 64 x 64 "suppresses"
// bits among them by ballot, one wave settles the 64 in order, and every later place is tested against the kept ones.
__global__ __launch_bounds__(kT) void nms_kernel(const float* __restrict__ iou, const float* __restrict__ scores,
                                                 const unsigned char* __restrict__ valid, unsigned char* __restrict__ keep, int N, float thr) {
    __shared__ unsigned long long s_key[SKIMI_NMS_MAX], s_rows[64], s_kept;
    __shared__ unsigned short s_order[SKIMI_NMS_MAX];
    __shared__ unsigned char s_supp[SKIMI_NMS_MAX];
    __shared__ int s_nvalid;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* io = iou + (size_t)blockIdx.x * N * N;
    const size_t vec = (size_t)blockIdx.x * N;
    if (tid == 0) s_nvalid = 0;
    __syncthreads();
    for (int i = tid; i < N; i += kT) {
        const float s = scores[vec + i];
        const bool ok = s == s && (!valid || valid[vec + i]);
        const unsigned bits = __float_as_uint(s == 0.f ? 0.f : s);   // -0 is 0
        const unsigned mono = (bits & 0x80000000u) ? ~bits : bits | 0x80000000u;   // >= 0x007FFFFF for every number
        s_key[i] = ((unsigned long long)(ok ? mono : 0u) << 32) | (0xFFFFFFFFu - (unsigned)i);
        s_supp[i] = 0;
        keep[vec + i] = 0;
        if (ok) atomicAdd(&s_nvalid, 1);
    }
    __syncthreads();
    for (int i = tid; i < N; i += kT) {
        const unsigned long long k = s_key[i];
        int rank = 0;
        for (int jj = 0; jj < N; ++jj) rank += s_key[jj] > k;
        s_order[rank] = (unsigned short)i;   // the keys are distinct: a permutation
    }
    __syncthreads();
    const int nv = s_nvalid;   // the entries that may be kept are the first nv places
    for (int p0 = 0; p0 < nv; p0 += 64) {   // uniform trip count; s_supp is indexed by place
        const bool q_in = p0 + lane < nv;
        const int jq = q_in ? s_order[p0 + lane] : 0;
        for (int p = wave; p < 64; p += kT / 64) {
            const bool bit = p0 + p < nv && q_in && lane > p && io[(size_t)s_order[p0 + p] * N + jq] > thr;
            const unsigned long long m = __ballot(bit);
            if (lane == 0) s_rows[p] = m;
        }
        __syncthreads();
        if (wave == 0) {
            unsigned long long alive = __ballot(q_in && !s_supp[p0 + lane]), kept = 0;
            for (int p = 0; p < 64; ++p)
                if ((alive >> p) & 1ull) {
                    kept |= 1ull << p;
                    alive &= ~s_rows[p];
                }
            if (lane == 0) s_kept = kept;
            if ((kept >> lane) & 1ull) keep[vec + jq] = 1;
        }
        __syncthreads();
        const unsigned long long kept = s_kept;
        for (int q = p0 + 64 + tid; q < nv; q += kT) {
            if (s_supp[q]) continue;
            const int j = s_order[q];
            for (unsigned long long m = kept; m; m &= m - 1)
                if (io[(size_t)s_order[p0 + __builtin_ctzll(m)] * N + j] > thr) {
                    s_supp[q] = 1;
                    break;
                }
        }
        // the next round's first barrier stands between these writes of s_supp and its reads of them
    }
}

bool mask_shape_ok(int64_t B, int32_t H, int32_t W) {
    return B >= 1 && H >= 1 && W >= 1 && H <= SKIMI_MASK_MAX_SIDE && W <= SKIMI_MASK_MAX_SIDE && B * H * W < (1ll << 31);
}

}  // namespace

}  // namespace skimi

using namespace skimi;

extern "C" {

size_t skimi_mask_components_workspace_bytes(int64_t B, int32_t H, int32_t W) {
    if (!mask_shape_ok(B, H, W)) return 0;
    return (size_t)B * H * W * 4 + (size_t)B * cdiv((int64_t)H * W, kChunk) * 4;
}

int skimi_mask_components(const uint8_t* masks, int64_t B, int32_t H, int32_t W, int32_t connectivity, int32_t max_components,
                          int32_t* labels, int32_t* areas, int32_t* count, int64_t* stats, void* ws, size_t ws_bytes, void* stream) {
    SKIMI_CHECK_ARG(mask_shape_ok(B, H, W), "skimi_mask_components: B = %lld masks of %d x %d outside 1 <= H, W <= %d, B H W < 2^31",
                    (long long)B, W, H, SKIMI_MASK_MAX_SIDE);
    SKIMI_CHECK_ARG(connectivity == 4 || connectivity == 8, "skimi_mask_components: connectivity %d (4 or 8)", connectivity);
    SKIMI_CHECK_ARG(max_components >= 0 && B * max_components < (1ll << 31), "skimi_mask_components: max_components = %d", max_components);
    SKIMI_CHECK_ARG(masks && labels && areas && count && (stats || max_components == 0) && ws,
                    "skimi_mask_components: NULL masks, labels, areas, count, stats or workspace");
    SKIMI_CHECK_ARG(ws_bytes >= skimi_mask_components_workspace_bytes(B, H, W), "skimi_mask_components: workspace of %zu bytes, need %zu",
                    ws_bytes, skimi_mask_components_workspace_bytes(B, H, W));
    hipStream_t st = (hipStream_t)stream;
    const int HW = H * W, tilesX = (int)cdiv(W, kTileW), tilesY = (int)cdiv(H, kTileH), groups = (int)cdiv(HW, kChunk);
    const int64_t tiles = B * tilesX * tilesY;
    SKIMI_CHECK_ARG(tiles < (1ll << 31) && B * groups < (1ll << 31), "skimi_mask_components: %lld tiles", (long long)tiles);
    int* parent = static_cast<int*>(ws);
    unsigned* bc = reinterpret_cast<unsigned*>(parent + (size_t)B * HW);
    const int conn8 = connectivity == 8;
    SKIMI_HIP(hipMemsetAsync(areas, 0, (size_t)B * HW * 4, st));
    hipLaunchKernelGGL(cc_tile_kernel, dim3((unsigned)tiles), dim3(kT), 0, st, masks, parent, H, W, tilesX, tilesY, conn8);
    const int64_t items = (int64_t)(tilesY - 1) * W + (int64_t)(tilesX - 1) * H;
    if (items > 0) {
        const int sg = (int)cdiv(items, kT);
        hipLaunchKernelGGL(cc_seams_kernel, dim3((unsigned)(B * sg)), dim3(kT), 0, st, parent, H, W, tilesX, tilesY, conn8, sg);
    }
    hipLaunchKernelGGL(cc_area_kernel, dim3((unsigned)tiles), dim3(kT), 0, st, parent, areas, H, W, tilesX, tilesY);
    hipLaunchKernelGGL(cc_root_count_kernel, dim3((unsigned)(B * groups)), dim3(kT), 0, st, parent, bc, HW, groups);
    hipLaunchKernelGGL(cc_root_number_kernel, dim3((unsigned)(B * groups)), dim3(kT), 0, st, parent, bc, count, HW, groups);
    if (max_components > 0) {
        const int64_t rows = B * max_components;
        SKIMI_HIP(hipMemsetAsync(stats, 0, (size_t)rows * 7 * 8, st));
        hipLaunchKernelGGL(cc_label_kernel<true>, dim3((unsigned)tiles), dim3(kT), 0, st, parent, labels, areas,
                           reinterpret_cast<unsigned long long*>(stats), H, W, tilesX, tilesY, max_components);
        hipLaunchKernelGGL(cc_stats_finish_kernel, dim3((unsigned)cdiv(rows, kT)), dim3(kT), 0, st, reinterpret_cast<long long*>(stats),
                           (long)rows);
    } else {
        hipLaunchKernelGGL(cc_label_kernel<false>, dim3((unsigned)tiles), dim3(kT), 0, st, parent, labels, areas,
                           (unsigned long long*)nullptr, H, W, tilesX, tilesY, 0);
    }
    SKIMI_LAUNCH_CHECK();
    return SKIMI_OK;
}

int skimi_mask_edt(const uint8_t* masks, int64_t B, int32_t H, int32_t W, int32_t border_zero, int32_t* d2, float* dist, void* stream) {
    SKIMI_CHECK_ARG(mask_shape_ok(B, H, W), "skimi_mask_edt: B = %lld masks of %d x %d outside 1 <= H, W <= %d, B H W < 2^31", (long long)B, W,
                    H, SKIMI_MASK_MAX_SIDE);
    SKIMI_CHECK_ARG(masks && d2, "skimi_mask_edt: NULL masks or d2");
    const int groups = (int)cdiv(W, kT);
    hipLaunchKernelGGL(edt_columns_kernel, dim3((unsigned)(B * groups)), dim3(kT), 0, (hipStream_t)stream, masks, d2, H, W, groups,
                       border_zero != 0);
    hipLaunchKernelGGL(edt_rows_kernel, dim3((unsigned)(B * H)), dim3(kT), 0, (hipStream_t)stream, d2, dist, W, border_zero != 0);
    SKIMI_LAUNCH_CHECK();
    return SKIMI_OK;
}

int skimi_mask_argmax(const int32_t* d2, int64_t B, int32_t H, int32_t W, int32_t* xy, int32_t* best, void* stream) {
    SKIMI_CHECK_ARG(mask_shape_ok(B, H, W), "skimi_mask_argmax: B = %lld maps of %d x %d outside 1 <= H, W <= %d, B H W < 2^31", (long long)B,
                    W, H, SKIMI_MASK_MAX_SIDE);
    SKIMI_CHECK_ARG(d2 && xy && best, "skimi_mask_argmax: NULL d2, xy or best");
    hipLaunchKernelGGL(argmax_kernel, dim3((unsigned)B), dim3(1024), 0, (hipStream_t)stream, d2, xy, best, H * W, W);
    SKIMI_LAUNCH_CHECK();
    return SKIMI_OK;
}

int skimi_mask_pack(const uint8_t* masks, int64_t B, int64_t HW, uint64_t* words, void* stream) {
    SKIMI_CHECK_ARG(B >= 1 && HW >= 1 && HW <= (int64_t)SKIMI_MASK_MAX_SIDE * SKIMI_MASK_MAX_SIDE && B * HW < (1ll << 31),
                    "skimi_mask_pack: B = %lld masks of %lld pixels outside 1 <= pixels <= %d^2, B pixels < 2^31", (long long)B, (long long)HW,
                    SKIMI_MASK_MAX_SIDE);
    SKIMI_CHECK_ARG(masks && words, "skimi_mask_pack: NULL masks or words");
    const int64_t nw = cdiv(HW, 64);
    const int groups = (int)cdiv(nw, kPackWords);
    hipLaunchKernelGGL(pack_kernel, dim3((unsigned)(B * groups)), dim3(kT), 0, (hipStream_t)stream, masks,
                       reinterpret_cast<unsigned long long*>(words), (long)HW, (long)nw, groups);
    SKIMI_LAUNCH_CHECK();
    return SKIMI_OK;
}

int skimi_mask_boxes(const uint64_t* words, int64_t B, int32_t H, int32_t W, int32_t* xyxy, int32_t* area, void* stream) {
    SKIMI_CHECK_ARG(mask_shape_ok(B, H, W), "skimi_mask_boxes: B = %lld masks of %d x %d outside 1 <= H, W <= %d, B H W < 2^31", (long long)B,
                    W, H, SKIMI_MASK_MAX_SIDE);
    SKIMI_CHECK_ARG(words && xyxy && area, "skimi_mask_boxes: NULL words, xyxy or area");
    hipLaunchKernelGGL(boxes_kernel, dim3((unsigned)B), dim3(1024), 0, (hipStream_t)stream, reinterpret_cast<const unsigned long long*>(words),
                       xyxy, area, H, W, (long)cdiv((int64_t)H * W, 64));
    SKIMI_LAUNCH_CHECK();
    return SKIMI_OK;
}

int skimi_mask_iou(const uint64_t* a, const uint64_t* b, int32_t T, int32_t N, int32_t M, int64_t words, float* iou, int32_t* inter,
                   int32_t* uni, void* stream) {
    SKIMI_CHECK_ARG(T >= 1 && T <= 65535 && N >= 1 && M >= 1 && cdiv(N, kPairs) <= 65535 && (int64_t)T * N * M < (1ll << 31),
                    "skimi_mask_iou: T = %d, N = %d, M = %d outside 1 <= T <= 65535, 1 <= N, M, T N M < 2^31", T, N, M);
    SKIMI_CHECK_ARG(words >= 1 && words <= (int64_t)SKIMI_MASK_MAX_SIDE * SKIMI_MASK_MAX_SIDE / 64, "skimi_mask_iou: %lld words a mask",
                    (long long)words);
    SKIMI_CHECK_ARG(a && b && iou && inter && uni, "skimi_mask_iou: NULL a, b, iou, inter or union");
    const dim3 grid((unsigned)cdiv(M, kPairs), (unsigned)cdiv(N, kPairs), (unsigned)T);
    hipLaunchKernelGGL(iou_kernel, grid, dim3(kT), 0, (hipStream_t)stream, reinterpret_cast<const unsigned long long*>(a),
                       reinterpret_cast<const unsigned long long*>(b), iou, inter, uni, N, M, (long)words);
    SKIMI_LAUNCH_CHECK();
    return SKIMI_OK;
}

int skimi_nms_greedy(const float* iou, const float* scores, const uint8_t* valid, int32_t T, int32_t N, float iou_threshold, uint8_t* keep,
                     void* stream) {
    SKIMI_CHECK_ARG(T >= 1 && N >= 1 && N <= SKIMI_NMS_MAX, "skimi_nms_greedy: T = %d problems of N = %d outside 1 <= T, 1 <= N <= %d", T, N,
                    SKIMI_NMS_MAX);
    SKIMI_CHECK_ARG(iou && scores && keep, "skimi_nms_greedy: NULL iou, scores or keep");
    hipLaunchKernelGGL(nms_kernel, dim3((unsigned)T), dim3(kT), 0, (hipStream_t)stream, iou, scores, valid, keep, N, iou_threshold);
    SKIMI_LAUNCH_CHECK();
    return SKIMI_OK;
}

}  // extern "C"
