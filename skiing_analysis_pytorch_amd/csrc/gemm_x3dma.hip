// bf16x3 (fp32-accurate) MFMA contraction with LDS-DMA staging, for the fp32-path heads (wide DPT
// convs) whose operands live in HBM PRE-SPLIT into bf16:
//     x = hi + lo,  hi = bf16(x),  lo = bf16(x - hi)      acc += Alo*Whi + Ahi*Wlo + Ahi*Whi
// The generic kernel (gemm.hip, NSPLIT = 3) splits fp32 operands in registers for every tile that
// touches them (a 3x3 conv re-splits each activation 9 x N/128 times) and stages through VGPRs.
// Here the split is done once (weights at finalize, activations by split_records_kernel) into
// 128-byte records [hi 32 | lo 32] per (row, 32-element K-slice), which stream global -> LDS with
// global_load_lds_dwordx4 a whole cache line per row; implicit-im2col gather = per-lane source
// pixel offset, padding taps read a zero page; epilogue shared with gemm.hip (bias / act /
// LayerScale / residuals / row remaps).
#include <stdlib.h>

#include <algorithm>

#include "common.h"
#include "env.h"
#include "gemm_epilogue.h"
#include "gfx950.h"

namespace skimi {

// fp32 [rows, C] (row stride ld) -> hi, lo bf16 planes [rows, C] contiguous
__global__ __launch_bounds__(256) void split_planes_kernel(const float* __restrict__ x, long ld, long rows, int C,
                                                           unsigned short* __restrict__ hi, unsigned short* __restrict__ lo) {
    const int C4 = C / 4;
    const long total = rows * C4;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long r = i / C4;
        const int c = (int)(i - r * C4) * 4;
        const float4 v = *reinterpret_cast<const float4*>(x + r * ld + c);
        const float f[4] = {v.x, v.y, v.z, v.w};
        bf16x4 h, l;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const unsigned short hb = f2bf(f[k]);
            h[k] = (short)hb;
            l[k] = (short)f2bf(f[k] - bf2f(hb));
        }
        *reinterpret_cast<bf16x4*>(hi + r * C + c) = h;
        *reinterpret_cast<bf16x4*>(lo + r * C + c) = l;
    }
}

int split_planes_launch(const float* x, long ld, long rows, int C, void* hi, void* lo, hipStream_t st) {
    SKIMI_CHECK_ARG(C % 4 == 0 && ld % 4 == 0, "split_planes: C and ld must be multiples of 4");
    const long total = rows * (C / 4);
    const int blocks = (int)std::max<long>(1, std::min<long>(cdiv(total, 256), 65536));
    hipLaunchKernelGGL(split_planes_kernel, dim3(blocks), dim3(256), 0, st, x, ld, rows, C, (unsigned short*)hi,
                       (unsigned short*)lo);
    SKIMI_LAUNCH_CHECK();
    return SKIMI_OK;
}

// fp32 [rows, C] (row stride ld) -> records [rows][ceil(C / 32)][hi 32 | lo 32] bf16: the hi and lo
// halves of a 32-element K-slice are one 128-byte line, so every staging access of the kernel
// below is a whole cache line (as separate planes a K-tile of 32 is 64-byte pieces, which the
// L2 -> LDS path moves at half the rate: tools/dma_depth.hip, 55 vs 101 GB/s per CU).  A ragged
// last slice is zero-filled.  zpage: optional 256 bytes to clear (zero page of the conv gather).
__global__ __launch_bounds__(256) void split_records_kernel(const float* __restrict__ x, long ld, long rows, int C,
                                                            unsigned short* __restrict__ rec, uint4* __restrict__ zpage) {
    if (zpage != nullptr && blockIdx.x == 0 && threadIdx.x < 16) zpage[threadIdx.x] = uint4{0, 0, 0, 0};
    const int S = (C + 31) / 32;          // slices per row
    const long total = rows * S * 8;      // one thread per 4 elements
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long rs = i >> 3;           // (row, slice)
        const int c = (int)(i & 7) * 4;   // element within the slice
        const long r = rs / S;
        const int col = (int)(rs - r * S) * 32 + c;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (col < C) v = *reinterpret_cast<const float4*>(x + r * ld + col);   // C % 4 == 0
        const float f[4] = {v.x, v.y, v.z, v.w};
        bf16x4 h, l;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const unsigned short hb = f2bf(f[k]);
            h[k] = (short)hb;
            l[k] = (short)f2bf(f[k] - bf2f(hb));
        }
        *reinterpret_cast<bf16x4*>(rec + rs * 64 + c) = h;
        *reinterpret_cast<bf16x4*>(rec + rs * 64 + 32 + c) = l;
    }
}

int split_records_launch(const float* x, long ld, long rows, int C, void* rec, hipStream_t st, void* zpage) {
    SKIMI_CHECK_ARG(C % 4 == 0 && ld % 4 == 0, "split_records: C and ld must be multiples of 4");
    const long total = rows * ((C + 31) / 32) * 8;
    const int blocks = (int)std::max<long>(1, std::min<long>(cdiv(total, 256), 65536));
    hipLaunchKernelGGL(split_records_kernel, dim3(blocks), dim3(256), 0, st, x, ld, rows, C, (unsigned short*)rec,
                       (uint4*)zpage);
    SKIMI_LAUNCH_CHECK();
    return SKIMI_OK;
}

struct X3Rec {
    const char* a;      // A records: [rows][Cp / 32][hi 32 | lo 32] bf16
    const char* w;      // W records: [N][Kp / 32][hi 32 | lo 32]
    const char* zero;   // >= 128 zero bytes behind the A records (padding taps of the conv gather)
    long a_row_bytes;   // bytes of one A row (pixel) = 4 * Cp
    long w_row_bytes;   // bytes of one W row = 4 * Kp
    long a_bias;        // conv: lane offsets are biased so that a window starting in the padding stays >= 0
};

// bf16x3 MFMA contraction, single-stream loop (same structure as gemm256w4_kernel): 256x256 tile,
// 4 waves (one per SIMD), each a 128x128 quadrant = 256 accumulator registers, every wave
// software-pipelining its own stream with ONE workgroup barrier per K-tile.  Per k-step of 16:
// 16 fragment reads (A hi/lo x 4 row blocks, W hi/lo x 4 column blocks) feed 48 MFMAs, issued
// term-major (all lo*hi, all hi*lo, all hi*hi) so that no MFMA waits for the accumulator of the
// one before it.
//
// LDS: ring of ten 16-KiB slots; a K-tile (BK = 32) is four pieces of 128 rows x 128 B (a row =
// one record, hi | lo): q = 0,1 the A rows of wave row 0 / 1, q = 2,3 the W rows of wave column
// 0 / 1; piece q of K-tile kt sits in slot (4 kt + q) mod 10, so the A pieces of K-tile kt+2 go
// out a whole K-tile early:
//   k-step 0 of kt : read (kt, k-step 1); issue A pieces of kt+2   -> the slots K-tile kt-1's W left
//   k-step 1 of kt : lgkmcnt(0), vmcnt(8) = all of kt+1 landed, barrier (= K-tile kt released),
//                    read (kt+1, k-step 0); issue W pieces of kt+2 -> K-tile kt's A slots
// A wave-instruction of LDS-DMA writes 8 rows x 128 B linearly; the bank swizzle (16-B chunk ^=
// (row >> 1) & 7) is applied to the per-lane SOURCE address and again on the ds_read_b128; the lo
// half of a fragment is the hi half's address ^ 64.  Staging addresses are (wave-uniform 64-bit
// base) + (per-lane unsigned 32-bit offset): the K-tile / tap part goes into the base on the
// scalar unit, a padding-tap lane only swaps its offset for the zero page's.
//
// M16 (SKIMI_X3_MFMA=16, the default): the quadrant is 8 x 8 tiles of 16x16 (256 accumulator registers again) and a
// K-tile is ONE k-step of 32 = 192 v_mfma_f32_16x16x32_bf16, the same MFMA cycles: on this shape the chip holds a
// higher clock (profiles/r04_peaks.json).  Operand map: row l & 15, 16-B chunk l >> 4 of the 64-B hi half (the
// records' K-slice is exactly one k-step), lo chunk = hi ^ 64; the source swizzle is unchanged (16 consecutive rows
// see chunk ^ 0..7 twice each: conflict-free).  Double-buffering a k-step's 32 fragments (128 VGPRs) next to 256
// accumulators does not fit, so the K-tile runs as three 64-MFMA phases, term by term, and a fragment group (8
// fragments = 32 VGPRs) is re-read as soon as its last phase is done:
//   phase 1  AL.WH : lgkmcnt(0); read AH, WL of kt;  issue A pieces of kt+2   -> the slots K-tile kt-1's W left
//   phase 2  AH.WH : lgkmcnt(0), vmcnt(8) = all of kt+1 landed, barrier (= K-tile kt released);
//                    read AL of kt+1; issue W pieces of kt+2 -> K-tile kt's A slots
//   phase 3  AH.WL : read WH of kt+1
// so at most four groups (128 VGPRs) are live, and every accumulator sees its three MFMAs 64 instructions apart.  The
// MFMAs are inline asm on AGPR-pinned accumulators, as in gemm256w4_kernel<.., M16> (gemm256.hip): the builtin makes
// hipcc shuttle accumulators between the register files.
template <int AMODE, int ABL = 0, bool M16 = false>   // a_mode of the launch (0 plain rows, 1 tap-major, 2 slice-major
                      // gather), compile-time: the K-tile body must stay one straight-line scheduling region.  ABL:
                      // timing ablations (bit 0 no staging, bit 1 no fragment reads, bit 2 no MFMAs)
__global__ __launch_bounds__(256, 1) void gemm_x3w4_kernel(const GemmArgs p, const X3Rec pl) {
    constexpr int BM = 256, BN = 256, BK = 32, RB = 128, PIECE = 128 * RB, NSLOT = 10;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1, wc = wave & 1;
    const int l31 = lane & 31, lh = lane >> 5;

    const int id = xcd_contiguous_id(blockIdx.x, p.ntm * p.ntn);
    const int tm = id / p.ntn, tn = id - tm * p.ntn;
    const int m0 = tm * BM;
    int n0 = tn * BN;
    // the gather window of this tile (wave-uniform): the launch's, or (FOLD) the one of the tile's output phase
    constexpr bool FOLD = AMODE == 3;
    int gKH = p.KH, gKW = p.KW, gpy = p.pad, gpx = p.pad, gstride = p.stride, gdil = p.dil, gOH = p.OH, gOW = p.OW;
    int nkt = (p.K + BK - 1) / BK;
    const char* wbase = pl.w;
    long w_row_bytes = pl.w_row_bytes;
    int fp = 0, fq = 0;   // FOLD: output phase (y mod s, x mod s) of this tile
    if constexpr (FOLD) {
        // A stride-s transposed conv followed by a 3x3 conv, as s x s small convs on the coarse map: column tile
        // tn = (phase, 256 channels of it).  Along an axis phase 0 reads coarse pixels {-1, 0}, phase s-1 {0, +1},
        // the others {0}; the weights are the phases' [ps_C][taps * cC] matrices (slice-major K) one after another.
        const int s = p.ps_s, ntc = (p.ps_C + BN - 1) / BN;
        const int f = tn / ntc;
        n0 = (tn - f * ntc) * BN;
        fp = f / s;
        fq = f - fp * s;
        gKH = (fp == 0 || fp == s - 1) ? 2 : 1;
        gKW = (fq == 0 || fq == s - 1) ? 2 : 1;
        gpy = fp == 0 ? 1 : 0;
        gpx = fq == 0 ? 1 : 0;
        gstride = 1; gdil = 1; gOH = p.cH; gOW = p.cW;
        // taps of the phases before this one: every phase row above holds (s + 2) column taps per row tap
        const int taps_before = (fp + (fp > 0 ? 1 : 0)) * (s + 2) + gKH * (fq + (fq > 0 ? 1 : 0));
        wbase += (long)taps_before * p.ps_C * p.cC * 4;
        w_row_bytes = (long)gKH * gKW * p.cC * 4;
        nkt = gKH * gKW * (p.cC / 32);
    }
    // records output: the 256 zero bytes behind them (the consumer's padding taps)
    if (p.out_rec != nullptr && blockIdx.x == 0 && tid < 16)
        reinterpret_cast<uint4*>(p.out_rec + (long)p.M * (FOLD ? p.ps_s * p.ps_s : 1) * p.rec_row)[tid] = uint4{0, 0, 0, 0};

    // ---- staging: a piece is 16 wave-instructions of 8 rows x 128 B; this wave issues 4*wave + j ----
    unsigned a_off[2][4], w_off[2][4];
    unsigned a_ok[2][4];   // conv: bit t = tap t of this lane's window is inside the image
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int row = (4 * wave + j) * 8 + (lane >> 3);      // row within the piece
            const int c = (lane & 7) ^ ((row >> 1) & 7);           // source chunk of this lane's LDS chunk
            const int m = min(m0 + 128 * q + row, p.M - 1);
            a_ok[q][j] = ~0u;
            if (AMODE == 0) {
                a_off[q][j] = (unsigned)((long)m * pl.a_row_bytes + c * 16);
            } else {
                const int ohw = gOH * gOW;
                const int img = m / ohw;
                const int rem = m - img * ohw;
                const int oy = rem / gOW;
                const int iy0 = oy * gstride - gpy, ix0 = (rem - oy * gOW) * gstride - gpx;
                a_off[q][j] = (unsigned)((((long)img * p.cH + iy0) * p.cW + ix0) * pl.a_row_bytes + c * 16 + pl.a_bias);
                unsigned ok = 0;
                for (int ky = 0; ky < gKH; ++ky)
                    for (int kx = 0; kx < gKW; ++kx) {
                        const int iy = iy0 + ky * gdil, ix = ix0 + kx * gdil;
                        if (iy >= 0 && iy < p.cH && ix >= 0 && ix < p.cW) ok |= 1u << (ky * gKW + kx);
                    }
                a_ok[q][j] = ok;
            }
            w_off[q][j] = (unsigned)((long)min(n0 + 128 * q + row, p.N - 1) * w_row_bytes + c * 16);
        }
    // K-tiles are requested in order, so the (tap, channel slice) of the next one is kept as scalar
    // counters: no integer division in the loop
    int cur_tap = 0, cur_ky = 0, cur_kx = 0, cur_cs = 0;
    // wave-uniform: base of the next K-tile's A records, the zero page seen from it, and its tap
    struct ATile {
        const char* base;
        unsigned z;
        int tap;
    };
    auto a_tile = [&](int kt) {
        const int tap = cur_tap, tap_dy = cur_ky * gdil, tap_dx = cur_kx * gdil;
        const int cs = AMODE == 0 ? kt : cur_cs;
        if (AMODE == 2 || FOLD) {  // slice-major K: the taps of a 32-channel slice are consecutive K-tiles
            ++cur_tap;
            if (++cur_kx == gKW) { cur_kx = 0; ++cur_ky; }
            if (cur_tap == gKH * gKW) { cur_tap = 0; cur_ky = 0; ++cur_cs; }
        } else if (AMODE == 1) {   // tap-major K: the channel slices of a tap are consecutive K-tiles
            if (++cur_cs == p.cC / 32) {
                cur_cs = 0;
                ++cur_tap;
                if (++cur_kx == gKW) { cur_kx = 0; ++cur_ky; }
            }
        }
        const long kbytes = ((long)tap_dy * p.cW + tap_dx) * pl.a_row_bytes + (long)cs * 128 - (AMODE != 0 ? pl.a_bias : 0);
        const char* base = pl.a + kbytes;
        return ATile{base, (unsigned)(pl.zero - base), tap};
    };
    // one staging instruction: rows 8 (4 wave + j) .. + 7 of A piece q (wave row q) / W piece q (wave column q)
    auto dma_a = [&](const ATile& at, int q, int j, int slot) {
        if (ABL & 1) return;
        const bool ok = AMODE == 0 || ((a_ok[q][j] >> at.tap) & 1u) != 0;
        const unsigned o = ok ? a_off[q][j] : at.z + ((lane & 7) << 4);
        lds_dma16(at.base + (size_t)o, smem + slot * PIECE + (4 * wave + j) * 8 * RB);
    };
    auto dma_w = [&](int kt, int q, int j, int slot) {
        if (ABL & 1) return;
        lds_dma16(wbase + (long)kt * 128 + (size_t)w_off[q][j], smem + slot * PIECE + (4 * wave + j) * 8 * RB);
    };
    auto issue_a = [&](int kt, int slot0, int slot1) {
        const ATile at = a_tile(kt);
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int j = 0; j < 4; ++j) dma_a(at, q, j, q == 0 ? slot0 : slot1);
    };
    auto issue_w = [&](int kt, int slot0, int slot1) {
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int j = 0; j < 4; ++j) dma_w(kt, q, j, q == 0 ? slot0 : slot1);
    };
    auto slot = [&](int x) { return x >= NSLOT ? x - NSLOT : x; };
    // accumulators of this wave's quadrant: 32x32 tiles [row block i][column block j], or (M16) 16x16 tiles
    // [16-column block j][16-row block i]
    f32x16 acc[4][4];
    f32x4 acc16[8][8];
    // the epilogue's slab row pitch in floats: the 16x16 layout writes rows 4 (l >> 4) + r, four 16-lane groups 4 rows
    // apart, which a 128-float pitch puts on the same banks; 132 moves them 16 banks apart
    constexpr int SP = M16 ? 132 : 128;

    if constexpr (M16) {
    const int l15 = lane & 15;
    const int off16 = l15 * RB + (((lane >> 4) ^ ((l15 >> 1) & 7)) << 4);   // hi chunk; the lo chunk is at ^ 64
    bf16x8 ah[8], al[8], wh[8], wl[8];
    if (ABL & 2) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const bf16x8 c = {(short)lane, 1, 2, 3, 4, 5, 6, 7};
            ah[i] = al[i] = wh[i] = wl[i] = c;
        }
    }
    // 16-row block i of this wave's A piece (W = false) or W piece (W = true) of the K-tile at slot sb, hi or lo half
    auto rd = [&](int sb, bool W, bool lo, int i, bf16x8& f) {
        if (ABL & 2) return;
        const char* base = smem + slot(sb + (W ? 2 + wc : wr)) * PIECE + (off16 ^ (lo ? 64 : 0));
        f = *reinterpret_cast<const bf16x8*>(base + i * 16 * RB);
    };
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            acc16[j][i] = f32x4{0.f, 0.f, 0.f, 0.f};
            asm volatile("" : "+a"(acc16[j][i]));
        }
    asm volatile("s_nop 1");   // v_accvgpr_write -> first MFMA reading it as C
    // one phase: 64 MFMAs (column block outer), extra(g) placed after MFMA g (asm volatile + sched_barrier: source
    // order = issue order)
    auto phase = [&](const bf16x8 (&fa)[8], const bf16x8 (&fw)[8], auto&& extra) {
#pragma unroll
        for (int j = 0; j < 8; ++j)
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                if (!(ABL & 4)) asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+a"(acc16[j][i]) : "v"(fa[i]), "v"(fw[j]));
                extra(8 * j + i);
                __builtin_amdgcn_sched_barrier(0);
            }
    };

    // prologue: K-tiles 0 and 1 whole, then AL and WH of K-tile 0
    issue_a(0, 0, 1);
    issue_w(0, 2, 3);
    if (nkt > 1) {
        issue_a(1, 4, 5);
        issue_w(1, 6, 7);
        wait_vmcnt<16>();
    } else {
        wait_vmcnt<0>();
    }
    fenced_barrier();
    int sb = 0;   // slot of piece 0 of K-tile kt
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        rd(sb, false, true, i, al[i]);
        rd(sb, true, false, i, wh[i]);
    }
#define SKIMI_X3_HEAD()                       \
    do {                                      \
        wait_lgkmcnt0();                      \
        __builtin_amdgcn_sched_barrier(0);    \
    } while (0)
    // one K-tile: the fragment reads go one behind each of a phase's first MFMAs, the 8 staging instructions one behind
    // every second of the next 16.  N1 / N2: K-tiles kt+1 / kt+2 exist (literals; the last two K-tiles are peeled)
#define SKIMI_X3_KTILE16(N1, N2)                                                                   \
    do {                                                                                           \
        const int nsb = slot(sb + 4), s8 = slot(sb + 8), s9 = slot(sb + 9), s1 = slot(sb + 1);     \
        /* phase 1: AL.WH; read AH, WL of kt; A pieces of kt+2 */                                  \
        SKIMI_X3_HEAD();                                                                           \
        ATile at{};                                                                                \
        if (N2) at = a_tile(kt + 2);                                                               \
        phase(al, wh, [&](int g) {                                                                 \
            if (g < 8) rd(sb, false, false, g, ah[g]);                                             \
            else if (g < 16) rd(sb, true, true, g - 8, wl[g - 8]);                                 \
            else if (N2 && g < 32 && (g & 1)) {                                                    \
                const int d = (g - 16) >> 1;                                                       \
                dma_a(at, d >> 2, d & 3, (d >> 2) ? s9 : s8);                                      \
            }                                                                                      \
        });                                                                                        \
        /* phase 2: AH.WH; kt+1 landed, barrier; read AL of kt+1; W pieces of kt+2 */              \
        SKIMI_X3_HEAD();                                                                           \
        if (N1) {                                                                                  \
            if (N2) wait_vmcnt<8>(); else wait_vmcnt<0>();                                         \
            fenced_barrier();                                                                      \
        }                                                                                          \
        phase(ah, wh, [&](int g) {                                                                 \
            if (N1 && g < 8) rd(nsb, false, true, g, al[g]);                                       \
            else if (N2 && g >= 8 && g < 24 && (g & 1)) {                                          \
                const int d = (g - 8) >> 1;                                                        \
                dma_w(kt + 2, d >> 2, d & 3, (d >> 2) ? s1 : sb);                                  \
            }                                                                                      \
        });                                                                                        \
        /* phase 3: AH.WL; read WH of kt+1 */                                                      \
        phase(ah, wl, [&](int g) {                                                                 \
            if (N1 && g < 8) rd(nsb, true, false, g, wh[g]);                                       \
        });                                                                                        \
        sb = nsb;                                                                                  \
    } while (0)
    int kt = 0;
    for (; kt + 2 < nkt; ++kt) SKIMI_X3_KTILE16(true, true);
    if (kt + 1 < nkt) {
        SKIMI_X3_KTILE16(true, false);
        ++kt;
    }
    SKIMI_X3_KTILE16(false, false);
#undef SKIMI_X3_KTILE16
#undef SKIMI_X3_HEAD
    // 12 states: last MFMA's D -> the epilogue's v_accvgpr_read; the pins make every accumulator a value of THIS
    // point, so that hipcc reads none of them out between the MFMAs
    asm volatile("s_nop 7\n\ts_nop 4");
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
        for (int i = 0; i < 8; ++i) asm volatile("" : "+a"(acc16[j][i]));
    } else {

    // ---- fragment reads: row block i of this wave's A piece / W piece, k-step s ----
    const int t = lh ^ ((l31 >> 1) & 7);
    const int lane_off = l31 * RB;
    bf16x8 ah0[4], al0[4], wh0[4], wl0[4], ah1[4], al1[4], wh1[4], wl1[4];
    if (ABL & 2) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const bf16x8 c = {(short)lane, 1, 2, 3, 4, 5, 6, 7};
            ah0[i] = al0[i] = wh0[i] = wl0[i] = ah1[i] = al1[i] = wh1[i] = wl1[i] = c;
        }
    }
    auto read = [&](int sb, int s, bf16x8 (&ah)[4], bf16x8 (&al)[4], bf16x8 (&wh)[4], bf16x8 (&wl)[4]) {
        if (ABL & 2) return;
        const int x = ((2 * s) ^ t) << 4;   // hi chunk; the lo chunk is at x ^ 64
        const char* pa = smem + slot(sb + wr) * PIECE + lane_off;
        const char* pw = smem + slot(sb + 2 + wc) * PIECE + lane_off;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            ah[i] = *reinterpret_cast<const bf16x8*>(pa + i * 32 * RB + x);
            al[i] = *reinterpret_cast<const bf16x8*>(pa + i * 32 * RB + (x ^ 64));
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            wh[i] = *reinterpret_cast<const bf16x8*>(pw + i * 32 * RB + x);
            wl[i] = *reinterpret_cast<const bf16x8*>(pw + i * 32 * RB + (x ^ 64));
        }
    };

#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
#define SKIMI_X3_MFMA(AH, AL, WH, WL)                                                                             \
    do {                                                                                                           \
        if (ABL & 4) break;                                                                                        \
        _Pragma("unroll") for (int j = 0; j < 4; ++j) _Pragma("unroll") for (int i = 0; i < 4; ++i)                \
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(AL[i], WH[j], acc[i][j], 0, 0, 0);                 \
        _Pragma("unroll") for (int j = 0; j < 4; ++j) _Pragma("unroll") for (int i = 0; i < 4; ++i)                \
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(AH[i], WL[j], acc[i][j], 0, 0, 0);                 \
        _Pragma("unroll") for (int j = 0; j < 4; ++j) _Pragma("unroll") for (int i = 0; i < 4; ++i)                \
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(AH[i], WH[j], acc[i][j], 0, 0, 0);                 \
    } while (0)
#define SKIMI_X3_HEAD()                       \
    do {                                      \
        wait_lgkmcnt0();                      \
        __builtin_amdgcn_sched_barrier(0);    \
    } while (0)
    // 16 fragment reads behind the first 8 MFMAs, NDMA staging instructions behind the next 2 NDMA
#define SKIMI_X3_TAIL(NDMA)                                                        \
    do {                                                                           \
        _Pragma("unroll") for (int g = 0; g < 8; ++g) {                            \
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                     \
            __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);                     \
        }                                                                          \
        _Pragma("unroll") for (int g = 0; g < NDMA; ++g) {                         \
            __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);                     \
            __builtin_amdgcn_sched_group_barrier(0x010, 1, 0);                     \
        }                                                                          \
        __builtin_amdgcn_sched_group_barrier(0x008, 40 - 2 * NDMA, 0);             \
        __builtin_amdgcn_sched_barrier(0);                                         \
    } while (0)

    // prologue: K-tiles 0 and 1 whole
    issue_a(0, 0, 1);
    issue_w(0, 2, 3);
    if (nkt > 1) {
        issue_a(1, 4, 5);
        issue_w(1, 6, 7);
        wait_vmcnt<16>();
    } else {
        wait_vmcnt<0>();
    }
    fenced_barrier();
    int sb = 0;   // slot of piece 0 of K-tile kt
    read(sb, 0, ah0, al0, wh0, wl0);
#define SKIMI_X3_KTILE(N1, N2)                                                      \
    do {                                                                            \
        const int nsb = slot(sb + 4);                                               \
        /* k-step 0 */                                                              \
        SKIMI_X3_HEAD();                                                            \
        read(sb, 1, ah1, al1, wh1, wl1);                                            \
        if (N2) issue_a(kt + 2, slot(sb + 8), slot(sb + 9));                        \
        SKIMI_X3_MFMA(ah0, al0, wh0, wl0);                                          \
        SKIMI_X3_TAIL((N2 ? 8 : 0));                                                \
        /* k-step 1 */                                                              \
        SKIMI_X3_HEAD();                                                            \
        if (N1) {                                                                   \
            if (N2) wait_vmcnt<8>(); else wait_vmcnt<0>();                          \
            fenced_barrier();                                                       \
            read(nsb, 0, ah0, al0, wh0, wl0);                                       \
            if (N2) issue_w(kt + 2, sb, slot(sb + 1));                              \
        }                                                                           \
        SKIMI_X3_MFMA(ah1, al1, wh1, wl1);                                          \
        if (N1) SKIMI_X3_TAIL((N2 ? 8 : 0)); else __builtin_amdgcn_sched_barrier(0); \
        sb = nsb;                                                                   \
    } while (0)
    int kt = 0;
    for (; kt + 2 < nkt; ++kt) SKIMI_X3_KTILE(true, true);
    if (kt + 1 < nkt) {
        SKIMI_X3_KTILE(true, false);
        ++kt;
    }
    SKIMI_X3_KTILE(false, false);
#undef SKIMI_X3_KTILE
#undef SKIMI_X3_TAIL
#undef SKIMI_X3_HEAD
#undef SKIMI_X3_MFMA
    }
    wait_lgkmcnt0();
    fenced_barrier();   // nobody reads operand pieces any more: the epilogue slabs alias slots 0..4

    // ---- epilogue: per-wave 32-row x 128-column passes through a private LDS slab (row pitch SP) ----
    float* stg = reinterpret_cast<float*>(smem) + wave * (32 * SP);
    // pass i: the accumulators of rows 32 i .. + 31 of the quadrant -> the slab.  32x32: lane l holds column l & 31,
    // rows 8 (r >> 2) + 4 (l >> 5) + (r & 3); 16x16: column l & 15, rows 4 (l >> 4) + r
    auto to_slab = [&](int i) {
        if constexpr (M16) {
            const int l15 = lane & 15, lq = lane >> 4;
            // pinned here, in each epilogue variant: otherwise hipcc reads all 256 accumulators out into VGPRs ahead of
            // the variant switch, and spills
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int j = 0; j < 8; ++j) asm volatile("" : "+a"(acc16[j][2 * i + b]));
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int j = 0; j < 8; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r) stg[(16 * b + 4 * lq + r) * SP + 16 * j + l15] = acc16[j][2 * i + b][r];
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) stg[((r & 3) + 8 * (r >> 2) + 4 * lh) * SP + j * 32 + l31] = acc[i][j][r];
        }
    };
    const int n = n0 + wc * 128 + 4 * (lane & 31);
    if constexpr (FOLD) {
        // Pixel-shuffle store of the tile's phase: coarse pixel m = (img, cy, cx) -> fine pixel (s cy + fp, s cx + fq),
        // one whole channel row per pixel.  The bias is beta[class][n]: the transposed conv's bias seen through the 3x3
        // taps that stay inside the fine map, class = 3 * (0 inside | 1 top row | 2 bottom row) + the same for columns.
        // It is a per-row 16-byte load from a 9-row table (like a residual), so border tiles take the same
        // branch-free path as interior ones.  Dispatch admits only fp32 out / records, bias, ReLU or no activation.
        const int s = p.ps_s, cW = p.cW, cH = p.cH;
        const float lo1 = p.act == SKIMI_ACT_RELU ? 0.f : -__builtin_inff();
        float* out = reinterpret_cast<float*>(p.out);
        const long fine_w = (long)cW * s;
        auto fine_row = [&](int r, int cx) { return ((long)r * s + fp) * fine_w + (long)cx * s + fq; };   // r = img * cH + cy
        auto beta_off = [&](int cy, int cx) {
            const int yc = (fp == 0 && cy == 0) ? 1 : (fp == s - 1 && cy == cH - 1) ? 2 : 0;
            const int xc = (fq == 0 && cx == 0) ? 1 : (fq == s - 1 && cx == cW - 1) ? 2 : 0;
            return (yc * 3 + xc) * p.ps_C;
        };
        if (m0 + BM <= p.M && n0 + BN <= p.N) {   // block-uniform
            // this lane's rows are lh + 2 k of the wave's 128, in order: (r, cy, cx) advance by two pixels per row
            // (cW >= 2, checked at dispatch), so no row pays an integer division
            const int mb = m0 + wr * 128 + lh;
            int r = mb / cW, cx = mb - r * cW, cy = r % cH;
#define SKIMI_X3_FOLD_PASS(HAS_OUT, HAS_REC)                                                                       \
    _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                                \
        to_slab(i);                                                                                                \
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");                                                     \
        wait_lgkmcnt0();                                                                                           \
        _Pragma("unroll") for (int half = 0; half < 2; ++half) {                                                   \
            float4 v[8], bs[8];                                                                                    \
            long orow[8];                                                                                          \
            _Pragma("unroll") for (int it = 0; it < 8; ++it)                                                       \
                v[it] = *reinterpret_cast<const float4*>(&stg[(half * 16 + it * 2 + lh) * SP + 4 * (lane & 31)]);  \
            _Pragma("unroll") for (int it = 0; it < 8; ++it) {                                                     \
                orow[it] = fine_row(r, cx);                                                                        \
                bs[it] = *reinterpret_cast<const float4*>(p.bias + beta_off(cy, cx) + n);                          \
                cx += 2;                                                                                           \
                const bool wrap = cx >= cW;                                                                        \
                cx -= wrap ? cW : 0;                                                                               \
                r += wrap ? 1 : 0;                                                                                 \
                cy += wrap ? 1 : 0;                                                                                \
                cy = cy == cH ? 0 : cy;                                                                            \
            }                                                                                                      \
            _Pragma("unroll") for (int it = 0; it < 8; ++it) {                                                     \
                const float4 y = make_float4(fmaxf(v[it].x + bs[it].x, lo1), fmaxf(v[it].y + bs[it].y, lo1),       \
                                             fmaxf(v[it].z + bs[it].z, lo1), fmaxf(v[it].w + bs[it].w, lo1));      \
                if (HAS_OUT) *reinterpret_cast<float4*>(out + orow[it] * p.ldo + n) = y;                           \
                if (HAS_REC) store_rec4(p, orow[it], n, y.x, y.y, y.z, y.w);                                       \
            }                                                                                                      \
        }                                                                                                          \
        wait_lgkmcnt0();                                                                                           \
    }
            // compile-time variants, as below: a uniform branch inside the unrolled passes costs a vmcnt(0) per store
            switch ((out ? 2 : 0) | (p.out_rec ? 1 : 0)) {
                case 3: SKIMI_X3_FOLD_PASS(true, true) break;
                case 2: SKIMI_X3_FOLD_PASS(true, false) break;
                case 1: SKIMI_X3_FOLD_PASS(false, true) break;
                default: break;
            }
#undef SKIMI_X3_FOLD_PASS
            return;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            to_slab(i);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            wait_lgkmcnt0();
#pragma unroll 1
            for (int it = 0; it < 16; ++it) {
                const int row_l = it * 2 + lh;
                const int m = m0 + wr * 128 + i * 32 + row_l;
                if (m >= p.M || n >= p.N) continue;
                const float4 v = *reinterpret_cast<const float4*>(&stg[row_l * SP + 4 * (lane & 31)]);
                const int r = m / cW, cx = m - r * cW, cy = r % cH;
                const float4 b = *reinterpret_cast<const float4*>(p.bias + beta_off(cy, cx) + n);
                const float4 y = make_float4(fmaxf(v.x + b.x, lo1), fmaxf(v.y + b.y, lo1), fmaxf(v.z + b.z, lo1), fmaxf(v.w + b.w, lo1));
                const long orow = fine_row(r, cx);
                if (out) *reinterpret_cast<float4*>(out + orow * p.ldo + n) = y;
                if (p.out_rec) store_rec4(p, orow, n, y.x, y.y, y.z, y.w);
            }
            wait_lgkmcnt0();
        }
        return;
    }
    // Interior tiles of the common case (fp32 rows, bias, ReLU before / after one fp32 residual): a
    // straight-line path, 8 rows of loads and stores in flight per lane (the checked loop below
    // pays a vmcnt(0) per row: stores share the counter with loads and hipcc cannot count across
    // its branches).  Measured on the 148x148 DPT convs: 400 -> ~200 us of a 1.8 ms launch.
    const bool relu_ok = (p.act == SKIMI_ACT_NONE || p.act == SKIMI_ACT_RELU) &&
                         (p.post_act == SKIMI_ACT_NONE || p.post_act == SKIMI_ACT_RELU);
    const bool fast = p.vec4 && p.store_mode == 0 && p.out_rpb == 0 && p.out_off == 0 && p.out2 == nullptr &&
                      p.out_dtype == SKIMI_F32 && p.gamma == nullptr && relu_ok && (p.resid != nullptr || p.resid2 == nullptr) &&
                      (p.resid == nullptr || p.resid_dtype == SKIMI_F32) &&
                      m0 + BM <= p.M && n0 + BN <= p.N;   // block-uniform
    if (fast) {
        const float lo1 = p.act == SKIMI_ACT_RELU ? 0.f : -__builtin_inff();
        const float lo2 = p.post_act == SKIMI_ACT_RELU ? 0.f : -__builtin_inff();
        float4 bs = make_float4(0.f, 0.f, 0.f, 0.f);
        if (p.bias) bs = *reinterpret_cast<const float4*>(p.bias + n);
        const float* rs = reinterpret_cast<const float*>(p.resid);
        const float* rs2 = reinterpret_cast<const float*>(p.resid2);
        float* out = reinterpret_cast<float*>(p.out);
        // residual row of output row m (row_map's remap, branch-free: rows_per_batch 0 = one batch of all rows)
        const int rpb = p.resid_rpb > 0 ? p.resid_rpb : 0x7fffffff;
        auto res_row = [&](long m) {
            const int b = (int)m / rpb;
            return ((long)b * p.resid_bs + ((int)m - b * rpb) + p.resid_off) * p.ldr;
        };
#define SKIMI_X3_EPI_PASS(HAS_RES, HAS_OUT, HAS_REC)                                                                                 \
    _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                                \
        to_slab(i);                                                                                                \
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");                                                     \
        wait_lgkmcnt0();                                                                                           \
        _Pragma("unroll") for (int half = 0; half < 2; ++half) {                                                   \
            const long mrow = m0 + wr * 128 + i * 32 + half * 16 + lh;                                             \
            float4 v[8], rr[8], r2[8];                                                                             \
            _Pragma("unroll") for (int it = 0; it < 8; ++it)                                                       \
                v[it] = *reinterpret_cast<const float4*>(&stg[(half * 16 + it * 2 + lh) * SP + 4 * (lane & 31)]);  \
            if (HAS_RES) _Pragma("unroll") for (int it = 0; it < 8; ++it)                                          \
                rr[it] = *reinterpret_cast<const float4*>(rs + res_row(mrow + it * 2) + n);                       \
            if (HAS_RES == 2) _Pragma("unroll") for (int it = 0; it < 8; ++it)                                     \
                r2[it] = *reinterpret_cast<const float4*>(rs2 + (mrow + it * 2) * p.ldr2 + n);                     \
            _Pragma("unroll") for (int it = 0; it < 8; ++it) {                                                     \
                float4 y = make_float4(fmaxf(v[it].x + bs.x, lo1), fmaxf(v[it].y + bs.y, lo1),                     \
                                       fmaxf(v[it].z + bs.z, lo1), fmaxf(v[it].w + bs.w, lo1));                    \
                if (HAS_RES) { y.x += rr[it].x; y.y += rr[it].y; y.z += rr[it].z; y.w += rr[it].w; }               \
                if (HAS_RES == 2) { y.x += r2[it].x; y.y += r2[it].y; y.z += r2[it].z; y.w += r2[it].w; }          \
                y = make_float4(fmaxf(y.x, lo2), fmaxf(y.y, lo2), fmaxf(y.z, lo2), fmaxf(y.w, lo2));               \
                if (HAS_OUT) *reinterpret_cast<float4*>(out + (mrow + it * 2) * p.ldo + n) = y;                    \
                if (HAS_REC) store_rec4(p, mrow + it * 2, n, y.x, y.y, y.z, y.w);                                  \
            }                                                                                                      \
        }                                                                                                          \
        wait_lgkmcnt0();                                                                                           \
    }
        // compile-time variants: a uniform branch inside the unrolled passes would cost a vmcnt(0) per store
        const int variant = (rs2 ? 8 : rs ? 4 : 0) | (out ? 2 : 0) | (p.out_rec ? 1 : 0);
        switch (variant) {
            case 11: SKIMI_X3_EPI_PASS(2, true, true) break;
            case 10: SKIMI_X3_EPI_PASS(2, true, false) break;
            case 9: SKIMI_X3_EPI_PASS(2, false, true) break;
            case 7: SKIMI_X3_EPI_PASS(1, true, true) break;
            case 6: SKIMI_X3_EPI_PASS(1, true, false) break;
            case 5: SKIMI_X3_EPI_PASS(1, false, true) break;
            case 3: SKIMI_X3_EPI_PASS(0, true, true) break;
            case 2: SKIMI_X3_EPI_PASS(0, true, false) break;
            case 1: SKIMI_X3_EPI_PASS(0, false, true) break;
            default: break;
        }
#undef SKIMI_X3_EPI_PASS
        return;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        to_slab(i);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        wait_lgkmcnt0();
#pragma unroll 1
        for (int it = 0; it < 16; ++it) {
            const int row_l = it * 2 + lh;
            const int m = m0 + wr * 128 + i * 32 + row_l;
            if (m >= p.M || n >= p.N) continue;
            const float4 v = *reinterpret_cast<const float4*>(&stg[row_l * SP + 4 * (lane & 31)]);
            const RowMap rm = row_map(p, m);
            if (p.vec4) {
                store_four(p, rm, n, v);
            } else {
                store_one(p, rm, n, v.x);
                if (n + 1 < p.N) store_one(p, rm, n + 1, v.y);
                if (n + 2 < p.N) store_one(p, rm, n + 2, v.z);
                if (n + 3 < p.N) store_one(p, rm, n + 3, v.w);
            }
        }
        wait_lgkmcnt0();
    }
}

// The same loop for 128-column tiles (the 256 -> 128 channel conv of the DPT heads): wave (wr, wc)
// owns 128 rows x 64 columns (4 x 2 MFMA tiles, 24 MFMAs and 12 fragment reads per k-step); a
// K-tile is three pieces (A rows of wave row 0 / 1, the 128 W rows), the ring holds nine slots =
// three whole K-tiles: K-tile kt+3 is requested into K-tile kt's slots right after the barrier that
// releases them, so two K-tiles (96 KiB) are in flight while one is multiplied.  M16: the three-phase K-tile of
// gemm_x3w4_kernel on 8 x 4 tiles of 16x16.
template <int AMODE, bool M16 = false>
__global__ __launch_bounds__(256, 1) void gemm_x3w4n_kernel(const GemmArgs p, const X3Rec pl) {
    constexpr int BM = 256, BN = 128, BK = 32, RB = 128, PIECE = 128 * RB, NSLOT = 9;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1, wc = wave & 1;
    const int l31 = lane & 31, lh = lane >> 5;

    const int id = xcd_contiguous_id(blockIdx.x, p.ntm * p.ntn);
    const int tm = id / p.ntn, tn = id - tm * p.ntn;
    const int m0 = tm * BM, n0 = tn * BN;
    const int nkt = (p.K + BK - 1) / BK;
    // records output: the 256 zero bytes behind them (the consumer's padding taps)
    if (p.out_rec != nullptr && blockIdx.x == 0 && tid < 16)
        reinterpret_cast<uint4*>(p.out_rec + (long)p.M * p.rec_row)[tid] = uint4{0, 0, 0, 0};

    // ---- staging (see gemm_x3w4_kernel): a piece is 16 wave-instructions of 8 rows x 128 B ----
    unsigned a_off[2][4], w_off[4];
    unsigned a_ok[2][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int row = (4 * wave + j) * 8 + (lane >> 3);
        const int c = (lane & 7) ^ ((row >> 1) & 7);
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int m = min(m0 + 128 * q + row, p.M - 1);
            a_ok[q][j] = ~0u;
            if (AMODE == 0) {
                a_off[q][j] = (unsigned)((long)m * pl.a_row_bytes + c * 16);
            } else {
                const int ohw = p.OH * p.OW;
                const int img = m / ohw;
                const int rem = m - img * ohw;
                const int oy = rem / p.OW;
                const int iy0 = oy * p.stride - p.pad, ix0 = (rem - oy * p.OW) * p.stride - p.pad;
                a_off[q][j] = (unsigned)((((long)img * p.cH + iy0) * p.cW + ix0) * pl.a_row_bytes + c * 16 + pl.a_bias);
                unsigned ok = 0;
                for (int ky = 0; ky < p.KH; ++ky)
                    for (int kx = 0; kx < p.KW; ++kx) {
                        const int iy = iy0 + ky * p.dil, ix = ix0 + kx * p.dil;
                        if (iy >= 0 && iy < p.cH && ix >= 0 && ix < p.cW) ok |= 1u << (ky * p.KW + kx);
                    }
                a_ok[q][j] = ok;
            }
        }
        w_off[j] = (unsigned)((long)min(n0 + row, p.N - 1) * pl.w_row_bytes + c * 16);
    }
    int cur_tap = 0, cur_ky = 0, cur_kx = 0, cur_cs = 0;
    struct ATile {
        const char* base;
        unsigned z;
        int tap;
    };
    auto a_tile = [&](int kt) {
        const int tap = cur_tap, tap_dy = cur_ky * p.dil, tap_dx = cur_kx * p.dil;
        const int cs = AMODE == 0 ? kt : cur_cs;
        if (AMODE == 2) {
            ++cur_tap;
            if (++cur_kx == p.KW) { cur_kx = 0; ++cur_ky; }
            if (cur_tap == p.KH * p.KW) { cur_tap = 0; cur_ky = 0; ++cur_cs; }
        } else if (AMODE == 1) {
            if (++cur_cs == p.cC / 32) {
                cur_cs = 0;
                ++cur_tap;
                if (++cur_kx == p.KW) { cur_kx = 0; ++cur_ky; }
            }
        }
        const long kbytes = ((long)tap_dy * p.cW + tap_dx) * pl.a_row_bytes + (long)cs * 128 - (AMODE != 0 ? pl.a_bias : 0);
        const char* base = pl.a + kbytes;
        return ATile{base, (unsigned)(pl.zero - base), tap};
    };
    auto dma_a = [&](const ATile& at, int q, int j, int slot) {
        const bool ok = AMODE == 0 || ((a_ok[q][j] >> at.tap) & 1u) != 0;
        const unsigned o = ok ? a_off[q][j] : at.z + ((lane & 7) << 4);
        lds_dma16(at.base + (size_t)o, smem + slot * PIECE + (4 * wave + j) * 8 * RB);
    };
    auto dma_w = [&](int kt, int j, int slot) {
        lds_dma16(pl.w + (long)kt * 128 + (size_t)w_off[j], smem + slot * PIECE + (4 * wave + j) * 8 * RB);
    };
    // all three pieces of K-tile kt -> slots s0 (A rows 0..127), s1 (A rows 128..255), s2 (W rows)
    auto issue = [&](int kt, int s0, int s1, int s2) {
        const ATile at = a_tile(kt);
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int j = 0; j < 4; ++j) dma_a(at, q, j, q == 0 ? s0 : s1);
#pragma unroll
        for (int j = 0; j < 4; ++j) dma_w(kt, j, s2);
    };
    auto slot = [&](int x) { return x >= NSLOT ? x - NSLOT : x; };
    // accumulators of this wave's 128 x 64: 32x32 tiles [row block i][column block j], or (M16) 16x16 tiles
    // [16-column block j][16-row block i]
    f32x16 acc[4][2];
    f32x4 acc16[4][8];
    constexpr int SP = M16 ? 68 : 64;   // slab row pitch in floats (see gemm_x3w4_kernel)

    if constexpr (M16) {
    // M16: the three-phase K-tile of gemm_x3w4_kernel on 8 x 4 tiles of 16x16 (96 MFMAs per K-tile, 12 + 8 + 4
    // fragment reads); K-tile kt+3 goes out in phase 2, right after the barrier that releases K-tile kt's slots
    const int l15 = lane & 15;
    const int off16 = l15 * RB + (((lane >> 4) ^ ((l15 >> 1) & 7)) << 4);
    bf16x8 ah[8], al[8], wh[4], wl[4];
    auto rd_a = [&](int sb, bool lo, int i, bf16x8& f) {
        f = *reinterpret_cast<const bf16x8*>(smem + slot(sb + wr) * PIECE + (off16 ^ (lo ? 64 : 0)) + i * 16 * RB);
    };
    auto rd_w = [&](int sb, bool lo, int j, bf16x8& f) {
        f = *reinterpret_cast<const bf16x8*>(smem + slot(sb + 2) * PIECE + (off16 ^ (lo ? 64 : 0)) + (wc * 64 + j * 16) * RB);
    };
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            acc16[j][i] = f32x4{0.f, 0.f, 0.f, 0.f};
            asm volatile("" : "+a"(acc16[j][i]));
        }
    asm volatile("s_nop 1");
    auto phase = [&](const bf16x8 (&fa)[8], const bf16x8 (&fw)[4], auto&& extra) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+a"(acc16[j][i]) : "v"(fa[i]), "v"(fw[j]));
                extra(8 * j + i);
                __builtin_amdgcn_sched_barrier(0);
            }
    };

    issue(0, 0, 1, 2);
    if (nkt > 1) issue(1, 3, 4, 5);
    if (nkt > 2) issue(2, 6, 7, 8);
    if (nkt > 2) wait_vmcnt<24>(); else if (nkt > 1) wait_vmcnt<12>(); else wait_vmcnt<0>();
    fenced_barrier();
    int sb = 0;   // slot of piece 0 of K-tile kt
#pragma unroll
    for (int i = 0; i < 8; ++i) rd_a(sb, true, i, al[i]);
#pragma unroll
    for (int j = 0; j < 4; ++j) rd_w(sb, false, j, wh[j]);
#define SKIMI_X3N_HEAD()                      \
    do {                                      \
        wait_lgkmcnt0();                      \
        __builtin_amdgcn_sched_barrier(0);    \
    } while (0)
    // N1 / N2 / N3: K-tiles kt+1 / kt+2 / kt+3 exist (literals; the last three K-tiles are peeled)
#define SKIMI_X3N_KTILE16(N1, N2, N3)                                                              \
    do {                                                                                           \
        const int nsb = slot(sb + 3), s1 = slot(sb + 1), s2 = slot(sb + 2);                        \
        /* phase 1: AL.WH; read AH, WL of kt */                                                    \
        SKIMI_X3N_HEAD();                                                                          \
        phase(al, wh, [&](int g) {                                                                 \
            if (g < 8) rd_a(sb, false, g, ah[g]);                                                  \
            else if (g < 12) rd_w(sb, true, g - 8, wl[g - 8]);                                     \
        });                                                                                        \
        /* phase 2: AH.WH; kt+1 landed, barrier; read AL of kt+1; K-tile kt+3 -> kt's slots */     \
        SKIMI_X3N_HEAD();                                                                          \
        ATile at{};                                                                                \
        if (N1) {                                                                                  \
            if (N2) wait_vmcnt<12>(); else wait_vmcnt<0>();                                        \
            fenced_barrier();                                                                      \
            if (N3) at = a_tile(kt + 3);                                                           \
        }                                                                                          \
        phase(ah, wh, [&](int g) {                                                                 \
            if (N1 && g < 8) rd_a(nsb, true, g, al[g]);                                            \
            else if (N3 && g >= 8 && (g & 1)) {                                                    \
                const int d = (g - 8) >> 1;                                                        \
                if (d < 8) dma_a(at, d >> 2, d & 3, (d >> 2) ? s1 : sb);                           \
                else dma_w(kt + 3, d - 8, s2);                                                     \
            }                                                                                      \
        });                                                                                        \
        /* phase 3: AH.WL; read WH of kt+1 */                                                      \
        phase(ah, wl, [&](int g) {                                                                 \
            if (N1 && g < 4) rd_w(nsb, false, g, wh[g]);                                           \
        });                                                                                        \
        sb = nsb;                                                                                  \
    } while (0)
    int kt = 0;
    for (; kt + 3 < nkt; ++kt) SKIMI_X3N_KTILE16(true, true, true);
    if (kt + 2 < nkt) {
        SKIMI_X3N_KTILE16(true, true, false);
        ++kt;
    }
    if (kt + 1 < nkt) {
        SKIMI_X3N_KTILE16(true, false, false);
        ++kt;
    }
    SKIMI_X3N_KTILE16(false, false, false);
#undef SKIMI_X3N_KTILE16
#undef SKIMI_X3N_HEAD
    asm volatile("s_nop 7\n\ts_nop 4");
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 8; ++i) asm volatile("" : "+a"(acc16[j][i]));
    } else {

    // ---- fragment reads ----
    const int t = lh ^ ((l31 >> 1) & 7);
    const int fa_off = l31 * RB, fw_off = (wc * 64 + l31) * RB;
    bf16x8 ah0[4], al0[4], wh0[2], wl0[2], ah1[4], al1[4], wh1[2], wl1[2];
    auto read = [&](int sb, int s, bf16x8 (&ah)[4], bf16x8 (&al)[4], bf16x8 (&wh)[2], bf16x8 (&wl)[2]) {
        const int x = ((2 * s) ^ t) << 4;
        const char* pa = smem + slot(sb + wr) * PIECE + fa_off;
        const char* pw = smem + slot(sb + 2) * PIECE + fw_off;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            ah[i] = *reinterpret_cast<const bf16x8*>(pa + i * 32 * RB + x);
            al[i] = *reinterpret_cast<const bf16x8*>(pa + i * 32 * RB + (x ^ 64));
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            wh[i] = *reinterpret_cast<const bf16x8*>(pw + i * 32 * RB + x);
            wl[i] = *reinterpret_cast<const bf16x8*>(pw + i * 32 * RB + (x ^ 64));
        }
    };

#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
#define SKIMI_X3N_MFMA(AH, AL, WH, WL)                                                                            \
    do {                                                                                                           \
        _Pragma("unroll") for (int j = 0; j < 2; ++j) _Pragma("unroll") for (int i = 0; i < 4; ++i)                \
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(AL[i], WH[j], acc[i][j], 0, 0, 0);                 \
        _Pragma("unroll") for (int j = 0; j < 2; ++j) _Pragma("unroll") for (int i = 0; i < 4; ++i)                \
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(AH[i], WL[j], acc[i][j], 0, 0, 0);                 \
        _Pragma("unroll") for (int j = 0; j < 2; ++j) _Pragma("unroll") for (int i = 0; i < 4; ++i)                \
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(AH[i], WH[j], acc[i][j], 0, 0, 0);                 \
    } while (0)
#define SKIMI_X3N_HEAD()                      \
    do {                                      \
        wait_lgkmcnt0();                      \
        __builtin_amdgcn_sched_barrier(0);    \
    } while (0)
    // 12 fragment reads behind the first 6 MFMAs, NDMA staging instructions one per MFMA after them
#define SKIMI_X3N_TAIL(NDMA)                                                       \
    do {                                                                           \
        _Pragma("unroll") for (int g = 0; g < 6; ++g) {                            \
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                     \
            __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);                     \
        }                                                                          \
        _Pragma("unroll") for (int g = 0; g < NDMA; ++g) {                         \
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                     \
            __builtin_amdgcn_sched_group_barrier(0x010, 1, 0);                     \
        }                                                                          \
        __builtin_amdgcn_sched_group_barrier(0x008, 18 - NDMA, 0);                 \
        __builtin_amdgcn_sched_barrier(0);                                         \
    } while (0)

    // prologue: the first three K-tiles
    issue(0, 0, 1, 2);
    if (nkt > 1) issue(1, 3, 4, 5);
    if (nkt > 2) issue(2, 6, 7, 8);
    if (nkt > 2) wait_vmcnt<24>(); else if (nkt > 1) wait_vmcnt<12>(); else wait_vmcnt<0>();
    fenced_barrier();
    int sb = 0;   // slot of piece 0 of K-tile kt
    read(sb, 0, ah0, al0, wh0, wl0);
    // N1 / N2 / N3: K-tiles kt+1 / kt+2 / kt+3 exist (literals; the last three K-tiles are peeled)
#define SKIMI_X3N_KTILE(N1, N2, N3)                                                 \
    do {                                                                            \
        const int nsb = slot(sb + 3);                                               \
        /* k-step 0 */                                                              \
        SKIMI_X3N_HEAD();                                                           \
        read(sb, 1, ah1, al1, wh1, wl1);                                            \
        SKIMI_X3N_MFMA(ah0, al0, wh0, wl0);                                         \
        SKIMI_X3N_TAIL(0);                                                          \
        /* k-step 1 */                                                              \
        SKIMI_X3N_HEAD();                                                           \
        if (N1) {                                                                   \
            if (N2) wait_vmcnt<12>(); else wait_vmcnt<0>();                         \
            fenced_barrier();                                                       \
            read(nsb, 0, ah0, al0, wh0, wl0);                                       \
            if (N3) issue(kt + 3, sb, slot(sb + 1), slot(sb + 2));                  \
        }                                                                           \
        SKIMI_X3N_MFMA(ah1, al1, wh1, wl1);                                         \
        if (N1) SKIMI_X3N_TAIL((N3 ? 12 : 0)); else __builtin_amdgcn_sched_barrier(0); \
        sb = nsb;                                                                   \
    } while (0)
    int kt = 0;
    for (; kt + 3 < nkt; ++kt) SKIMI_X3N_KTILE(true, true, true);
    if (kt + 2 < nkt) {
        SKIMI_X3N_KTILE(true, true, false);
        ++kt;
    }
    if (kt + 1 < nkt) {
        SKIMI_X3N_KTILE(true, false, false);
        ++kt;
    }
    SKIMI_X3N_KTILE(false, false, false);
#undef SKIMI_X3N_KTILE
#undef SKIMI_X3N_TAIL
#undef SKIMI_X3N_HEAD
#undef SKIMI_X3N_MFMA
    }
    wait_lgkmcnt0();
    fenced_barrier();   // nobody reads operand pieces any more: the epilogue slabs alias slots 0..2

    // ---- epilogue: per-wave 32-row x 64-column passes through a private LDS slab (row pitch SP) ----
    float* stg = reinterpret_cast<float*>(smem) + wave * (32 * SP);
    auto to_slab = [&](int i) {
        if constexpr (M16) {
            const int l15 = lane & 15, lq = lane >> 4;
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int j = 0; j < 4; ++j) asm volatile("" : "+a"(acc16[j][2 * i + b]));
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r) stg[(16 * b + 4 * lq + r) * SP + 16 * j + l15] = acc16[j][2 * i + b][r];
        } else {
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) stg[((r & 3) + 8 * (r >> 2) + 4 * lh) * SP + j * 32 + l31] = acc[i][j][r];
        }
    };
    const int n = n0 + wc * 64 + 4 * (lane & 15);
    const bool relu_ok = (p.act == SKIMI_ACT_NONE || p.act == SKIMI_ACT_RELU) &&
                         (p.post_act == SKIMI_ACT_NONE || p.post_act == SKIMI_ACT_RELU);
    const bool fast = p.vec4 && p.store_mode == 0 && p.out_rpb == 0 && p.out_off == 0 && p.out2 == nullptr &&
                      p.out_dtype == SKIMI_F32 && p.gamma == nullptr && relu_ok && (p.resid != nullptr || p.resid2 == nullptr) &&
                      (p.resid == nullptr || p.resid_dtype == SKIMI_F32) &&
                      m0 + BM <= p.M && n0 + BN <= p.N;   // block-uniform
    if (fast) {
        const float lo1 = p.act == SKIMI_ACT_RELU ? 0.f : -__builtin_inff();
        const float lo2 = p.post_act == SKIMI_ACT_RELU ? 0.f : -__builtin_inff();
        float4 bs = make_float4(0.f, 0.f, 0.f, 0.f);
        if (p.bias) bs = *reinterpret_cast<const float4*>(p.bias + n);
        const float* rs = reinterpret_cast<const float*>(p.resid);
        const float* rs2 = reinterpret_cast<const float*>(p.resid2);
        float* out = reinterpret_cast<float*>(p.out);
        // residual row of output row m (row_map's remap, branch-free: rows_per_batch 0 = one batch of all rows)
        const int rpb = p.resid_rpb > 0 ? p.resid_rpb : 0x7fffffff;
        auto res_row = [&](long m) {
            const int b = (int)m / rpb;
            return ((long)b * p.resid_bs + ((int)m - b * rpb) + p.resid_off) * p.ldr;
        };
#define SKIMI_X3N_EPI_PASS(HAS_RES, HAS_OUT, HAS_REC)                                                                                \
    _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                                \
        to_slab(i);                                                                                                \
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");                                                     \
        wait_lgkmcnt0();                                                                                           \
        const long mrow = m0 + wr * 128 + i * 32 + (lane >> 4);                                                    \
        float4 v[8], rr[8], r2[8];                                                                                 \
        _Pragma("unroll") for (int it = 0; it < 8; ++it)                                                           \
            v[it] = *reinterpret_cast<const float4*>(&stg[(it * 4 + (lane >> 4)) * SP + 4 * (lane & 15)]);         \
        if (HAS_RES) _Pragma("unroll") for (int it = 0; it < 8; ++it)                                              \
            rr[it] = *reinterpret_cast<const float4*>(rs + res_row(mrow + it * 4) + n);                           \
        if (HAS_RES == 2) _Pragma("unroll") for (int it = 0; it < 8; ++it)                                         \
            r2[it] = *reinterpret_cast<const float4*>(rs2 + (mrow + it * 4) * p.ldr2 + n);                         \
        _Pragma("unroll") for (int it = 0; it < 8; ++it) {                                                         \
            float4 y = make_float4(fmaxf(v[it].x + bs.x, lo1), fmaxf(v[it].y + bs.y, lo1),                         \
                                   fmaxf(v[it].z + bs.z, lo1), fmaxf(v[it].w + bs.w, lo1));                        \
            if (HAS_RES) { y.x += rr[it].x; y.y += rr[it].y; y.z += rr[it].z; y.w += rr[it].w; }                   \
            if (HAS_RES == 2) { y.x += r2[it].x; y.y += r2[it].y; y.z += r2[it].z; y.w += r2[it].w; }              \
            y = make_float4(fmaxf(y.x, lo2), fmaxf(y.y, lo2), fmaxf(y.z, lo2), fmaxf(y.w, lo2));                   \
            if (HAS_OUT) *reinterpret_cast<float4*>(out + (mrow + it * 4) * p.ldo + n) = y;                        \
            if (HAS_REC) store_rec4(p, mrow + it * 4, n, y.x, y.y, y.z, y.w);                                      \
        }                                                                                                          \
        wait_lgkmcnt0();                                                                                           \
    }
        const int variant = (rs2 ? 8 : rs ? 4 : 0) | (out ? 2 : 0) | (p.out_rec ? 1 : 0);
        switch (variant) {
            case 11: SKIMI_X3N_EPI_PASS(2, true, true) break;
            case 10: SKIMI_X3N_EPI_PASS(2, true, false) break;
            case 9: SKIMI_X3N_EPI_PASS(2, false, true) break;
            case 7: SKIMI_X3N_EPI_PASS(1, true, true) break;
            case 6: SKIMI_X3N_EPI_PASS(1, true, false) break;
            case 5: SKIMI_X3N_EPI_PASS(1, false, true) break;
            case 3: SKIMI_X3N_EPI_PASS(0, true, true) break;
            case 2: SKIMI_X3N_EPI_PASS(0, true, false) break;
            case 1: SKIMI_X3N_EPI_PASS(0, false, true) break;
            default: break;
        }
#undef SKIMI_X3N_EPI_PASS
        return;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        to_slab(i);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        wait_lgkmcnt0();
#pragma unroll 1
        for (int it = 0; it < 8; ++it) {
            const int row_l = it * 4 + (lane >> 4);
            const int m = m0 + wr * 128 + i * 32 + row_l;
            if (m >= p.M || n >= p.N) continue;
            const float4 v = *reinterpret_cast<const float4*>(&stg[row_l * SP + 4 * (lane & 15)]);
            const RowMap rm = row_map(p, m);
            if (p.vec4) {
                store_four(p, rm, n, v);
            } else {
                store_one(p, rm, n, v.x);
                if (n + 1 < p.N) store_one(p, rm, n + 1, v.y);
                if (n + 2 < p.N) store_one(p, rm, n + 2, v.z);
                if (n + 3 < p.N) store_one(p, rm, n + 3, v.w);
            }
        }
        wait_lgkmcnt0();
    }
}

static long x3_rows_in(const skimi_gemm_desc* d) { return d->a_mode == 0 ? (long)d->M : (long)d->cN * d->cH * d->cW; }
static long x3_cp(const skimi_gemm_desc* d) { return ((d->a_mode == 0 ? (long)d->K : (long)d->cC) + 31) / 32 * 32; }
static int x3_pad(const skimi_gemm_desc* d) { return d->a_mode == 3 ? 1 : d->pad; }   // a_mode 3: windows start at -1 or 0

size_t gemm_x3dma_scratch_bytes(const skimi_gemm_desc* d) {
    return (size_t)x3_rows_in(d) * x3_cp(d) * 4 + 256;   // A records + 256 zero bytes
}

// a desc qualifies when its weights also come as records (W_split), the caller lent scratch for
// the activation records, and the problem fills the chip with 256x256 tiles
bool gemm_x3dma_eligible(const skimi_gemm_desc* d) {
    if (d->prec != SKIMI_PREC_BF16X3 || d->W_split == nullptr) return false;
    if (d->a_dtype == SKIMI_F32) {
        if (d->x3_scratch == nullptr || d->x3_scratch_bytes < gemm_x3dma_scratch_bytes(d)) return false;
        if (d->lda % 4 != 0) return false;
    } else if (d->a_dtype == SKIMI_BF16X3_REC) {
        // the caller's zero page must lie behind the records, within reach of a 32-bit lane offset
        const long rec_bytes = (long)gemm_x3dma_scratch_bytes(d) - 256;
        const long dz = (const char*)d->x3_scratch - (const char*)d->A;
        if (d->x3_scratch == nullptr || d->x3_scratch_bytes < 256 || dz < rec_bytes || dz >= (1ll << 32) - (1 << 28)) return false;
        if (((uintptr_t)d->A & 127) != 0) return false;
    } else {
        return false;
    }
    const bool fold = d->a_mode == 3;   // phase-folded ConvTranspose + 3x3 conv: its gather and its store come together
    if (fold != (d->store_mode == 2)) return false;
    if (d->store_mode < 0 || d->store_mode > 2) return false;
    if (d->K % 4 != 0) return false;
    if (d->a_mode != 0 && (d->cC % 32 != 0 || d->KH * d->KW > 32)) return false;
    // 32-bit lane offsets from a scalar base
    const long kp = ((long)d->K + 31) / 32 * 32;
    const long bias = d->a_mode == 0 ? 0 : ((long)x3_pad(d) * d->cW + x3_pad(d)) * x3_cp(d) * 4;
    if ((long)gemm_x3dma_scratch_bytes(d) + bias >= (1ll << 32) || (long)d->N * kp * 4 >= (1ll << 32)) return false;
    if (d->a_mode == 1 || d->a_mode == 2) {
        // a padding-tap lane reaches the zero page as an UNSIGNED offset from its K-tile's base (A + tap offset - bias), so
        // every base must lie in front of the zero page.  A tap that starts behind the whole input (pad > cH with a
        // dilated window: all its lanes are padding) would put the base behind it: the generic kernel takes those
        const long rec_bytes = (long)gemm_x3dma_scratch_bytes(d) - 256;
        const long zero_off = d->a_dtype == SKIMI_BF16X3_REC ? (long)((const char*)d->x3_scratch - (const char*)d->A) : rec_bytes;
        const long last_base = ((long)(d->KH - 1) * d->dil * d->cW + (long)(d->KW - 1) * d->dil) * x3_cp(d) * 4 + x3_cp(d) * 4 - 128 - bias;
        if (last_base >= zero_off) return false;
    }
    if (fold) {
        // the 256-column loop only (a tile is one phase's channels), its epilogue's forms only
        if (d->ps_s < 2 || d->ps_C <= 128 || d->ps_C % 32 != 0 || d->N != d->ps_C || d->cW < 2 || d->bias == nullptr ||
            d->out_dtype != SKIMI_F32 || (d->act != SKIMI_ACT_NONE && d->act != SKIMI_ACT_RELU) || d->post_act != SKIMI_ACT_NONE ||
            d->gamma != nullptr || d->resid != nullptr || d->resid2 != nullptr || d->out2 != nullptr || d->ldo % 4 != 0 ||
            ((uintptr_t)d->out & 15) != 0 || ((uintptr_t)d->bias & 15) != 0)
            return false;
    }
    // enough 256-row tiles for most of the chip (one workgroup per CU).  Measured in the bench: the level
    // with 172 tiles (M = 43808) is already faster here than on the generic 128x128 kernel (17.38 vs
    // 17.18 frames/s at a threshold of 160 vs 200); below that the generic kernel's smaller tiles win.
    // (SKIMI_X3_MIN_TILES overrides the threshold: the tests run small shapes through these kernels)
    const long min_tiles = env_switch("SKIMI_X3_MIN_TILES", 160);
    const long tiles = cdiv(d->M, 256) * (d->N > 128 ? cdiv(d->N, 256) : 1) * (fold ? d->ps_s * d->ps_s : 1);
    return d->M >= (min_tiles <= 1 ? 256 : 4096) && d->N >= 96 && tiles >= min_tiles;
}

// MFMA shape of both loops (SKIMI_X3_MFMA = 16 | 32): v_mfma_f32_16x16x32_bf16 by default; read once, or per launch
// under SKIMI_ENV_DYNAMIC=1 (interleaved A/B timing in one process)
static bool x3_m16() {
    const int shape = (int)env_switch("SKIMI_X3_MFMA", 16);
    return shape != 32;
}

// the 256-column loop; a_mode 3: every output phase has its own column tiles
template <int AMODE, int ABL = 0>
static int launch_x3w4(GemmArgs& a, const X3Rec& pl, hipStream_t st, int phases = 1) {
    constexpr size_t lds = 10ull * 128 * 128;
    const int64_t ntm = cdiv(a.M, 256), ntn = cdiv(a.N, 256) * phases;
    return x3_m16() ? launch_tiles<gemm_x3w4_kernel<AMODE, ABL, true>>(a, st, lds, 256, ntm, ntn, "gemm_x3w4", pl)
                    : launch_tiles<gemm_x3w4_kernel<AMODE, ABL, false>>(a, st, lds, 256, ntm, ntn, "gemm_x3w4", pl);
}

// the 128-column loop (N <= 128)
template <int AMODE>
static int launch_x3w4n(GemmArgs& a, const X3Rec& pl, hipStream_t st) {
    constexpr size_t lds = 9ull * 128 * 128;
    const int64_t ntm = cdiv(a.M, 256), ntn = cdiv(a.N, 128);
    return x3_m16() ? launch_tiles<gemm_x3w4n_kernel<AMODE, true>>(a, st, lds, 256, ntm, ntn, "gemm_x3w4n", pl)
                    : launch_tiles<gemm_x3w4n_kernel<AMODE, false>>(a, st, lds, 256, ntm, ntn, "gemm_x3w4n", pl);
}

// d->x3_scratch: the A records (4 bytes per element of the A buffer, rows padded to 32) + 256 zero bytes
int gemm_x3dma_launch(GemmArgs& a, const skimi_gemm_desc* d, hipStream_t st) {
    const long rows_in = x3_rows_in(d), cp = x3_cp(d);
    const int Cw = d->a_mode == 0 ? d->K : d->cC;
    char* rec = (char*)d->x3_scratch;
    char* zpage = rec + rows_in * cp * 4;
    if (d->a_dtype == SKIMI_BF16X3_REC) {   // the producer already wrote records (and cleared its zero page)
        rec = (char*)d->A;
        zpage = (char*)d->x3_scratch;
    } else {
        int rc = split_records_launch((const float*)d->A, d->lda, rows_in, Cw, rec, st, zpage);
        if (rc) return rc;
    }
    X3Rec pl;
    pl.a = rec;
    pl.w = (const char*)d->W_split;
    pl.zero = zpage;
    pl.a_row_bytes = cp * 4;
    pl.w_row_bytes = ((long)d->K + 31) / 32 * 32 * 4;
    pl.a_bias = d->a_mode == 0 ? 0 : ((long)x3_pad(d) * d->cW + x3_pad(d)) * pl.a_row_bytes;
    a.dbg = 0;
    set_gemm_path(d->N <= 128 ? SKIMI_GEMM_PATH_X3DMA_NARROW : SKIMI_GEMM_PATH_X3DMA_WIDE, 0, x3_m16() ? 1 : 2, 0, 1);
    if (a.a_mode == 3) return launch_x3w4<3>(a, pl, st, d->ps_s * d->ps_s);
    if (d->N <= 128) {
        if (a.a_mode == 0) return launch_x3w4n<0>(a, pl, st);
        if (a.a_mode == 1) return launch_x3w4n<1>(a, pl, st);
        return launch_x3w4n<2>(a, pl, st);
    }
#ifdef SKIMI_ABLATIONS   // timing ablations (wrong results): only in a -DSKIMI_ABLATIONS build
#define SKIMI_X3_ABL_GO(AMODE)                                  \
    switch ((int)env_once("SKIMI_X3_ABL", 0)) {                 \
        case 1: return launch_x3w4<AMODE, 1>(a, pl, st);        \
        case 2: return launch_x3w4<AMODE, 2>(a, pl, st);        \
        case 3: return launch_x3w4<AMODE, 3>(a, pl, st);        \
        case 5: return launch_x3w4<AMODE, 5>(a, pl, st);        \
        case 6: return launch_x3w4<AMODE, 6>(a, pl, st);        \
        default: break;                                         \
    }
    if (a.a_mode == 0) SKIMI_X3_ABL_GO(0)
    if (a.a_mode == 2) SKIMI_X3_ABL_GO(2)
#undef SKIMI_X3_ABL_GO
#endif
    if (a.a_mode == 0) return launch_x3w4<0>(a, pl, st);
    if (a.a_mode == 1) return launch_x3w4<1>(a, pl, st);
    return launch_x3w4<2>(a, pl, st);
}

}  // namespace skimi
