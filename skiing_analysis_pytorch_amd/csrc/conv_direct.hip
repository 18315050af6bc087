// Direct 3x3 convolution, Cin % 32 == 0 -> 32 output channels, stride 1, pad 1, fp32-accurate
// (bf16 hi/lo planes, 3 MFMAs per product), channels-last.  The DPT heads end in such a layer at the
// full 518 x 518 resolution (dpt_head.py:224-235 scratch.output_conv2[0]: 128 -> 32).
//
// As an implicit-gather GEMM this layer is the worst case of gemm.hip: N = 32 gives no reuse of a
// staged A tile across column tiles, so every input element is fetched nine times through the
// L1 / L2 into registers (measured 6.6 TB/s of gather traffic, 1.5 ms per 8 frames).  Here a
// workgroup owns a 16 x 16 pixel tile: the 18 x 18 halo window of one 32-channel slice is brought
// into LDS once by LDS-DMA and all nine taps read it from there; the 9 x 32 x 32 weight slice is
// staged the same way and shared by the 8 waves.
//   * 8 waves, wave w = output rows 2w, 2w+1 of the tile (32 pixels = one MFMA row block);
//   * per 32-channel slice: 9 taps x 2 k-steps x {a_lo.w_hi, a_hi.w_lo, a_hi.w_hi} = 54
//     v_mfma_f32_32x32x16_bf16 per wave on one 32 x 32 accumulator;
//   * LDS rows are 64 B (32 bf16) per pixel / per (tap, cout); the 16-B chunk is XOR-swizzled on the DMA source and
//     on the ds_read_b128: by (cout >> 2) & 3 for the weights, by ((hx + 2 hy) >> 2) & 3 for the window, whose second
//     tile row is read with its columns rotated by two (conflict-free at the 18-pixel pitch: see the fragment addresses);
//   * double-buffered slices: 2 x (2 planes x 21 KiB window + 2 planes x 18 KiB weights) = 156 KiB;
//   * the epilogue stores straight from the accumulator layout: for every register 32 lanes hold
//     the 32 output channels of one pixel = one full 128-B line.
// The DPT heads launch it on the align-corners upsample of the coarse fp32 map, which the kernel then makes itself
// (conv_direct_n32_kernel<true>, conv_direct_n32_up_launch): the window planes are interpolated in LDS from the source
// samples the window touches, so the 2 x 2 bytes per element of [hi | lo] records are neither written nor read back.
#include "common.h"
#include "env.h"
#include "gfx950.h"
#include "kernels.h"
#include "vggt_kernels.h"

namespace skimi {

__device__ uint4 g_conv_zero_page[4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};

constexpr int CD_WIN = 18 * 18;            // halo window pixels
constexpr int CD_IN_PLANE = 21 * 1024;     // 324 px x 64 B rounded up to whole 1-KiB DMA pieces
constexpr int CD_W_PLANE = 9 * 32 * 64;    // 18 KiB
constexpr int CD_BUF = 2 * CD_IN_PLANE + 2 * CD_W_PLANE;

// weights [32][Cin][3][3] fp32 -> [Cin/32][plane hi|lo][tap][cout 32][32] bf16
__global__ void conv_direct_pack_kernel(const float* __restrict__ w, unsigned short* __restrict__ out, int Cin) {
    const long n = 32L * Cin * 9;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const int c32 = (int)(i % 32);
        const int co = (int)((i / 32) % 32);
        const int tap = (int)((i / 1024) % 9);
        const int cs = (int)(i / 9216);
        const float v = w[((long)co * Cin + cs * 32 + c32) * 9 + tap];
        const unsigned short hi = f2bf(v);
        const unsigned short lo = f2bf(v - bf2f(hi));
        const long base = (long)cs * 2 * 9216 + tap * 1024 + co * 32 + c32;
        out[base] = hi;
        out[base + 9216] = lo;
    }
}

int conv_direct_pack_launch(const float* w, unsigned short* out, int Cin, hipStream_t st) {
    SKIMI_CHECK_ARG(Cin % 32 == 0, "conv_direct: Cin %% 32 != 0");
    hipLaunchKernelGGL(conv_direct_pack_kernel, dim3(64), dim3(256), 0, st, w, out, Cin);
    SKIMI_LAUNCH_CHECK();
    return SKIMI_OK;
}

struct ConvDirectArgs {
    const unsigned short* in_hi;   // [F][H][W][C] bf16 planes of the fp32 input
    const unsigned short* in_lo;
    const unsigned short* w;       // conv_direct_pack_kernel layout
    const float* bias;             // [32] or null
    float* out;                    // [F][H][W][32]
    int F, H, W, C, relu, tiles_x, tiles_y;
    long px_stride;                // elements between pixels in a plane (C for separate planes, 2C for [hi | lo] pixel records)
    // UP: the input is the align-corners bilinear resize of src (+ the UV embedding), made in the window staging
    const float* src;              // [F][h][w][C] fp32
    const float* tabx;             // [W][C/2] and [H][C/2], or both null
    const float* taby;
    int h, w_src;
    float sy, sx;                  // (h - 1) / (H - 1), (w - 1) / (W - 1) as bilinear_ac_planes_kernel computes them
};

// UP's LDS: one pair of window planes, written by the interpolation; the weights, the fp32 source window ([12][12]
// pixels x 32 channels) and the UV rows ([24, 18 used][32 channels]: the tabx row of a window column below C / 2, the
// taby row of a window row from C / 2 on) double-buffered, all three by LDS-DMA one step ahead
constexpr int CU_SRC = 12;                               // source rows / columns a window may touch (checked at launch)
constexpr int CU_SRC_BUF = CU_SRC * CU_SRC * 128;        // 18 KiB
constexpr int CU_TAB_BUF = 3 * 1024;
constexpr int CU_W0 = 2 * CD_IN_PLANE;
constexpr int CU_SRC0 = CU_W0 + 2 * 2 * CD_W_PLANE;
constexpr int CU_TAB0 = CU_SRC0 + 2 * CU_SRC_BUF;
constexpr int CU_LDS = CU_TAB0 + 2 * CU_TAB_BUF;         // 156 KiB
static_assert(CU_LDS <= 160 * 1024, "conv_direct: the fused window staging does not fit the LDS");

// !UP: one tile per workgroup, gridDim.x = the number of tiles, the input planes in memory.
// UP: the grid is at most one workgroup per CU and workgroup b walks tiles b, b + gridDim.x, ...  (tile, slice) is one
// sequence of steps over the double buffers: the parity runs on across tiles (C / 32 may be odd), and the step that
// computes a tile's last slice stages slice 0 of the workgroup's next tile, so only the very first stage of a
// workgroup is exposed.  A step first interpolates its slice of the window from the staged source into the [hi | lo]
// planes (the arithmetic of bilinear_ac_planes_kernel through the same helpers; halo pixels outside the image are
// zeros, the conv's padding), meets a barrier that leaves the next step's DMA in flight, and then runs the same taps.
// A tile's stores are issued behind the barrier that ends its last slice and are first waited for by the vmcnt(0) that
// ends the next tile's slice 0, an interpolation and a slice of MFMAs later: nothing between the two waits.
// Every loop bound around a barrier is workgroup-uniform (t, ntiles, gridDim.x, nsl).  Per output the MFMA order is
// slice -> tap -> k-step -> lo.hi, hi.lo, hi.hi in both.
template <bool UP>
__global__ __launch_bounds__(512, 2) void conv_direct_n32_kernel(const ConvDirectArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, lh = lane >> 5;

    const int ntiles = p.F * p.tiles_y * p.tiles_x;
    const int nsl = p.C / 32;
    const unsigned short* zero = reinterpret_cast<const unsigned short*>(g_conv_zero_page);

    // ---- DMA plan: piece q of a kind goes to wave q % 8.  Window pieces (16 pixels x 64 B each) 0..20 per plane, weight
    //      pieces 0..17 per plane; UP: source pieces (8 pixels x 128 B each) 0..17 and UV pieces 0..2 on waves 7..5 ----
    const int nin = UP ? (wave < 2 ? 3 : 2) : (wave < 5 ? 3 : 2);   // pieces wave, wave + 8, wave + 16 below 18 / 21
    int f, y0, x0;                      // the tile that in_off[] belongs to
    int ys0 = 0, xs0 = 0;               // UP: the source sample of the staged window's first row / column
    long in_off[3];                     // element offset of this lane's source pixel (channel 0), -1 = outside the image
    int tab_row[2] = {0, 0};            // UP: element offset of this lane's tabx / taby row
    auto plan_tile = [&](int t) {
        x0 = (t % p.tiles_x) * 16;
        t /= p.tiles_x;
        y0 = (t % p.tiles_y) * 16;
        f = t / p.tiles_y;
        if constexpr (UP) {
            ys0 = bilinear_ac_tap(p.sy, max(y0 - 1, 0), p.h).i0;
            xs0 = bilinear_ac_tap(p.sx, max(x0 - 1, 0), p.w_src).i0;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const int sp = 8 * (wave + 8 * j) + (lane >> 3);
                const int ry = sp / CU_SRC, rx = sp - ry * CU_SRC;   // rows past 11 (pieces past 17) are not staged
                const int y = min(ys0 + ry, p.h - 1), x = min(xs0 + rx, p.w_src - 1);
                in_off[j] = (((long)f * p.h + y) * p.w_src + x) * p.C + (lane & 7) * 4;
            }
            const int i = min(8 * (7 - wave) + (lane >> 3), 17);
            tab_row[0] = min(max(x0 - 1 + i, 0), p.W - 1) * (p.C / 2);
            tab_row[1] = min(max(y0 - 1 + i, 0), p.H - 1) * (p.C / 2);
        } else {
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const int px = 16 * (wave + 8 * j) + (lane >> 2);
                const int hy = px / 18, hx = px - hy * 18;
                const int y = y0 - 1 + hy, x = x0 - 1 + hx;
                const int sc = (lane & 3) ^ (((hx + 2 * hy) >> 2) & 3);
                in_off[j] = -1;
                if (px < CD_WIN && y >= 0 && y < p.H && x >= 0 && x < p.W)
                    in_off[j] = (((long)f * p.H + y) * p.W + x) * p.px_stride + sc * 8;
            }
        }
    };
    int w_off[3];
    const int nw = wave < 2 ? 3 : 2;    // pieces wave, wave + 8, wave + 16 below 18
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int row = 16 * (wave + 8 * j) + (lane >> 2);
        const int sc = (lane & 3) ^ ((row >> 2) & 3);
        w_off[j] = row * 32 + sc * 8;
    }
    auto stage = [&](int buf, int s) {   // the bare builtin = lds_dma16 of gfx950.h, which moves this kernel's m0 writes
        char* base = smem + (UP ? 0 : buf * CD_BUF);
        if constexpr (UP) {
            char* sb = smem + CU_SRC0 + buf * CU_SRC_BUF;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                if (j < nin)   // wave-uniform
                    __builtin_amdgcn_global_load_lds((gbl_void*)(p.src + in_off[j] + s * 32), (lds_void*)(sb + (wave + 8 * j) * 1024),
                                                     16, 0, 0);
            }
            if (p.tabx != nullptr && wave >= 5) {
                const int half = p.C / 2, cg = s * 32 + (lane & 7) * 4;
                const float* e = cg < half ? p.tabx + tab_row[0] + cg : p.taby + tab_row[1] + (cg - half);
                __builtin_amdgcn_global_load_lds((gbl_void*)e, (lds_void*)(smem + CU_TAB0 + buf * CU_TAB_BUF + (7 - wave) * 1024), 16,
                                                 0, 0);
            }
        } else {
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                if (j < nin) {   // wave-uniform
                    const bool ok = in_off[j] >= 0;
                    const unsigned short* sh = ok ? p.in_hi + in_off[j] + s * 32 : zero;
                    const unsigned short* sl = ok ? p.in_lo + in_off[j] + s * 32 : zero;
                    char* dst = base + (wave + 8 * j) * 1024;
                    __builtin_amdgcn_global_load_lds((gbl_void*)sh, (lds_void*)dst, 16, 0, 0);
                    __builtin_amdgcn_global_load_lds((gbl_void*)sl, (lds_void*)(dst + CD_IN_PLANE), 16, 0, 0);
                }
            }
        }
        const unsigned short* ws = p.w + (long)s * 2 * 9216;
        char* wb = base + 2 * CD_IN_PLANE + (UP ? buf * 2 * CD_W_PLANE : 0);
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            if (j < nw) {
                char* dst = wb + (wave + 8 * j) * 1024;
                __builtin_amdgcn_global_load_lds((gbl_void*)(ws + w_off[j]), (lds_void*)dst, 16, 0, 0);
                __builtin_amdgcn_global_load_lds((gbl_void*)(ws + 9216 + w_off[j]), (lds_void*)(dst + CD_W_PLANE), 16, 0, 0);
            }
        }
    };
    // UP: slice s of the window of tile (ty0, tx0), whose staged source starts at (tys0, txs0), from buffer buf into the
    // planes: item i = 8 channels of window pixel i >> 2, 1296 items over 512 threads
    auto interpolate = [&](int buf, int s, int ty0, int tx0, int tys0, int txs0) {
        const char* sb = smem + CU_SRC0 + buf * CU_SRC_BUF;
        const char* tb = smem + CU_TAB0 + buf * CU_TAB_BUF;
        const bool add_e = p.tabx != nullptr;
#pragma unroll 1
        for (int i = tid; i < 4 * CD_WIN; i += 512) {
            const int px = i >> 2, c4 = i & 3;
            const int hy = px / 18, hx = px - hy * 18;
            const int Y = ty0 - 1 + hy, X = tx0 - 1 + hx;
            bf16x8 hi = {0, 0, 0, 0, 0, 0, 0, 0}, lo = {0, 0, 0, 0, 0, 0, 0, 0};
            if (Y >= 0 && Y < p.H && X >= 0 && X < p.W) {
                const BilinearTap ty = bilinear_ac_tap(p.sy, Y, p.h), tx = bilinear_ac_tap(p.sx, X, p.w_src);
                const int r0 = (ty.i0 - tys0) * CU_SRC, r1 = (ty.i1 - tys0) * CU_SRC, c0 = tx.i0 - txs0, c1 = tx.i1 - txs0;
                float p00[8], p01[8], p10[8], p11[8], e[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                auto ld8 = [&](const char* q, float* d) {
                    const float4 a = *reinterpret_cast<const float4*>(q), b = *reinterpret_cast<const float4*>(q + 16);
                    d[0] = a.x; d[1] = a.y; d[2] = a.z; d[3] = a.w; d[4] = b.x; d[5] = b.y; d[6] = b.z; d[7] = b.w;
                };
                ld8(sb + (r0 + c0) * 128 + c4 * 32, p00);
                ld8(sb + (r0 + c1) * 128 + c4 * 32, p01);
                ld8(sb + (r1 + c0) * 128 + c4 * 32, p10);
                ld8(sb + (r1 + c1) * 128 + c4 * 32, p11);
                if (add_e) ld8(tb + (s * 32 + c4 * 8 < p.C / 2 ? hx : hy) * 128 + c4 * 32, e);
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    short hb, lb;
                    bilinear_ac_split(ty, tx, p00[k], p01[k], p10[k], p11[k], add_e, e[k], hb, lb);
                    hi[k] = hb;
                    lo[k] = lb;
                }
            }
            char* dst = smem + px * 64 + ((c4 ^ (((hx + 2 * hy) >> 2) & 3)) << 4);
            *reinterpret_cast<bf16x8*>(dst) = hi;
            *reinterpret_cast<bf16x8*>(dst + CD_IN_PLANE) = lo;
        }
    };

    // ---- fragment addresses: lane (l31, lh) of wave w reads pixel (2w + (l31 >> 4) + dy, col(l31) + dx) ----
    // The window's row pitch is 18 pixels = 4.5 bank rows of 256 B, so the second tile row of a fragment sits two pixels off
    // the first inside a bank row.  Two measures make every ds_read_b128 conflict-free (checked against the instruction's
    // four 16-lane groups, MI355X_MICROARCH.md §LDS; the first version's key (px >> 2) & 3 was a 2-way conflict on every
    // A read): the chunk key follows u = hx + 2 hy, and the lanes of the second row take their columns rotated by two
    // (col = (l31 + 14) & 15), so that a lane group's sixteen u values are distinct mod 16.
    const int col = ((l31 & 15) + ((l31 >> 4) ? 14 : 0)) & 15;
    int a_off[9][2];
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
        const int dy = tap / 3, dx = tap - dy * 3;
        const int hy = 2 * wave + (l31 >> 4) + dy, hx = col + dx;
        const int px = hy * 18 + hx;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) a_off[tap][ks] = px * 64 + (((2 * ks + lh) ^ (((hx + 2 * hy) >> 2) & 3)) << 4);
    }
    int b_off[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) b_off[ks] = l31 * 64 + (((2 * ks + lh) ^ ((l31 >> 2) & 3)) << 4);

    // an ordinary load: requested ahead of every LDS-DMA and retired by the first barrier's vmcnt(0), so that its use in
    // the epilogue waits for nothing that is in flight there
    float bs = p.bias ? p.bias[l31] : 0.f;

    int t = blockIdx.x;   // < ntiles: the grid is never larger
    int par = 0;          // the LDS buffer of the step about to be computed
    plan_tile(t);
    stage(0, 0);
    __syncthreads();   // drains the LDS-DMA (vmcnt(0)) ahead of the barrier
    asm volatile("" : "+v"(bs));
    for (;;) {
        // this tile: plan_tile moves f, y0, x0, ys0, xs0 on to the next one in its last slice
        const int tf = f, ty0 = y0, tx0 = x0, tys0 = ys0, txs0 = xs0;
        const bool more = UP && ntiles - t > (int)gridDim.x;
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        for (int s = 0; s < nsl; ++s) {
            // UP interpolates first: with an LDS-DMA in flight hipcc puts a vmcnt(0) in front of the staging reads
            if constexpr (UP) interpolate(par, s, ty0, tx0, tys0, txs0);
            if (s + 1 < nsl) {
                stage(par ^ 1, s + 1);
            } else if (more) {
                plan_tile(t + (int)gridDim.x);
                stage(par ^ 1, 0);
            }
            if constexpr (UP) {
                wait_lgkmcnt0();    // the planes are written; the next step's DMA stays in flight across this barrier
                fenced_barrier();
            }
            const char* ih = smem + (UP ? 0 : par * CD_BUF);
            const char* wh = ih + 2 * CD_IN_PLANE + (UP ? par * 2 * CD_W_PLANE : 0);
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    const bf16x8 a_hi = *reinterpret_cast<const bf16x8*>(ih + a_off[tap][ks]);
                    const bf16x8 a_lo = *reinterpret_cast<const bf16x8*>(ih + CD_IN_PLANE + a_off[tap][ks]);
                    const bf16x8 w_hi = *reinterpret_cast<const bf16x8*>(wh + tap * 2048 + b_off[ks]);
                    const bf16x8 w_lo = *reinterpret_cast<const bf16x8*>(wh + CD_W_PLANE + tap * 2048 + b_off[ks]);
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_lo, w_hi, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_hi, w_lo, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_hi, w_hi, acc, 0, 0, 0);
                }
            }
            par ^= 1;
            __syncthreads();   // the next step's DMA has landed (vmcnt(0)); every wave is done reading this step's buffer
        }

        // ---- epilogue: register r of lane (cout = l31, lh) is MFMA row (r&3) + 8 (r>>2) + 4 lh of the wave's 32, i.e. pixel
        //      (row >> 4, column rotated back by two in the second tile row) ----
        const bool interior = ty0 + 16 <= p.H && tx0 + 16 <= p.W;   // block-uniform
        float* ob = p.out + ((long)tf * p.H * p.W) * 32 + l31;
        if (interior) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int pix = (r & 3) + 8 * (r >> 2) + 4 * lh;
                const int y = ty0 + 2 * wave + (pix >> 4), x = tx0 + (((pix & 15) + ((pix >> 4) ? 14 : 0)) & 15);
                float v = acc[r] + bs;
                if (p.relu) v = fmaxf(v, 0.f);
                ob[((long)y * p.W + x) * 32] = v;
            }
        } else {
#pragma unroll 1
            for (int r = 0; r < 16; ++r) {
                const int pix = (r & 3) + 8 * (r >> 2) + 4 * lh;
                const int y = ty0 + 2 * wave + (pix >> 4), x = tx0 + (((pix & 15) + ((pix >> 4) ? 14 : 0)) & 15);
                float v = acc[r] + bs;
                if (p.relu) v = fmaxf(v, 0.f);
                if (y < p.H && x < p.W) ob[((long)y * p.W + x) * 32] = v;
            }
        }
        if (!more) break;
        t += (int)gridDim.x;
    }
}

// compute units of the current device, asked once per device
static int cu_count(int* cus) {
    static std::atomic<int> seen[32];
    int dev = 0;
    SKIMI_HIP(hipGetDevice(&dev));
    int n = seen[dev & 31].load(std::memory_order_relaxed);
    if (n == 0) {
        SKIMI_HIP(hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev));
        SKIMI_CHECK_ARG(n > 0, "conv_direct: the device reports no compute units");
        seen[dev & 31].store(n, std::memory_order_relaxed);
    }
    *cus = n;
    return SKIMI_OK;
}

int conv_direct_n32_launch(const unsigned short* in_hi, const unsigned short* in_lo, const unsigned short* w_packed,
                           const float* bias, float* out, int F, int H, int W, int C, int relu, hipStream_t st,
                           long px_stride) {
    SKIMI_CHECK_ARG(in_hi && in_lo && w_packed && out, "conv_direct: null buffer");
    SKIMI_CHECK_ARG(C % 32 == 0 && C >= 32 && F > 0 && H > 0 && W > 0, "conv_direct: bad shape");
    SKIMI_CHECK_ARG((((uintptr_t)in_hi | (uintptr_t)in_lo | (uintptr_t)w_packed) & 15) == 0, "conv_direct: 16-B alignment");
    if (px_stride <= 0) px_stride = C;
    // every pixel holds C / 8 DMA chunks of 16 B: they must not reach into the next pixel, and each must be 16-B aligned
    SKIMI_CHECK_ARG(px_stride >= C, "conv_direct: px_stride < C");
    SKIMI_CHECK_ARG(px_stride % 8 == 0, "conv_direct: px_stride %% 8 != 0 (16-B aligned pixels)");
    constexpr size_t lds = 2ull * CD_BUF;
    SKIMI_LDS_OPT_IN(conv_direct_n32_kernel<false>, lds, "conv_direct");
    ConvDirectArgs a = {};
    a.in_hi = in_hi; a.in_lo = in_lo; a.w = w_packed; a.bias = bias; a.out = out;
    a.F = F; a.H = H; a.W = W; a.C = C; a.relu = relu;
    a.px_stride = px_stride;
    a.tiles_x = (int)cdiv(W, 16);
    a.tiles_y = (int)cdiv(H, 16);
    const long nblk = (long)F * a.tiles_x * a.tiles_y;
    SKIMI_CHECK_ARG(nblk < (1l << 31), "conv_direct: grid too large");
    hipLaunchKernelGGL(conv_direct_n32_kernel<false>, dim3((unsigned)nblk), dim3(512), lds, st, a);
    SKIMI_LAUNCH_CHECK();
    return SKIMI_OK;
}

// The window of a tile touches source samples i0(first pixel) .. i1(last pixel) on an axis: at most CU_SRC of them on
// every tile of both axes, or the fused launch is not for this shape.  The same taps as the kernel computes.
static bool up_axis_fits(int n_src, int n_out) {
    const float scale = n_out > 1 ? (float)(n_src - 1) / (float)(n_out - 1) : 0.f;
    for (int o = 0; o < n_out; o += 16) {
        const int first = o > 0 ? o - 1 : 0, last = o + 16 < n_out ? o + 16 : n_out - 1;
        if (bilinear_ac_tap(scale, last, n_src).i1 - bilinear_ac_tap(scale, first, n_src).i0 + 1 > CU_SRC) return false;
    }
    return true;
}

bool conv_direct_n32_up_eligible(int h, int w, int H, int W, int C) {
    return env_switch("SKIMI_DPT_TAIL_FUSED", 1) != 0 && C % 32 == 0 && C >= 32 && h > 0 && w > 0 && H > 0 && W > 0 &&
           up_axis_fits(h, H) && up_axis_fits(w, W);
}

int conv_direct_n32_up_launch(const float* src, int h, int w, const float* tabx, const float* taby,
                              const unsigned short* w_packed, const float* bias, float* out, int F, int H, int W, int C, int relu,
                              hipStream_t st) {
    SKIMI_CHECK_ARG(src && w_packed && out, "conv_direct: null buffer");
    SKIMI_CHECK_ARG(F > 0 && conv_direct_n32_up_eligible(h, w, H, W, C), "conv_direct: shape not eligible for the fused upsample");
    SKIMI_CHECK_ARG((((uintptr_t)src | (uintptr_t)w_packed | (uintptr_t)tabx | (uintptr_t)taby) & 15) == 0, "conv_direct: 16-B alignment");
    SKIMI_CHECK_ARG(tabx == nullptr || taby != nullptr, "fused uv pos embed needs both tables");
    ConvDirectArgs a = {};
    a.w = w_packed; a.bias = bias; a.out = out;
    a.F = F; a.H = H; a.W = W; a.C = C; a.relu = relu;
    a.src = src; a.tabx = tabx; a.taby = taby; a.h = h; a.w_src = w;
    a.sy = H > 1 ? (float)(h - 1) / (float)(H - 1) : 0.f;
    a.sx = W > 1 ? (float)(w - 1) / (float)(W - 1) : 0.f;
    a.tiles_x = (int)cdiv(W, 16);
    a.tiles_y = (int)cdiv(H, 16);
    const long nblk = (long)F * a.tiles_x * a.tiles_y;
    SKIMI_CHECK_ARG(nblk < (1l << 31), "conv_direct: grid too large");
    // one workgroup per CU (the LDS admits no second one); SKIMI_CONV_DIRECT_GRID caps the grid further, so that a small
    // shape makes one workgroup walk many tiles (tests, A/B runs)
    int cus = 0;
    const int rc = cu_count(&cus);
    if (rc != SKIMI_OK) return rc;
    long grid = nblk < cus ? nblk : cus;
    const long cap = env_switch("SKIMI_CONV_DIRECT_GRID", 0);
    if (cap > 0 && cap < grid) grid = cap;
    SKIMI_LDS_OPT_IN(conv_direct_n32_kernel<true>, CU_LDS, "conv_direct");
    hipLaunchKernelGGL(conv_direct_n32_kernel<true>, dim3((unsigned)grid), dim3(512), CU_LDS, st, a);
    SKIMI_LAUNCH_CHECK();
    return SKIMI_OK;
}

}  // namespace skimi
