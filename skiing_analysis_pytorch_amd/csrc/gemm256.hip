// 256x256-tile bf16 MFMA contraction with direct global->LDS staging (global_load_lds_dwordx4),
// the fast path of the aggregator / DINOv2 linears (plain rows, bf16 A and W, K % 64 == 0).
//
// Why a second kernel: the generic 128x128 kernel moves 64 FLOP per byte staged from L2; at
// MFMA speed that asks the 8 XCD L2s for more than they deliver.  A 256x256 tile doubles the
// reuse (128 FLOP/B), and LDS-DMA staging removes the VGPR round trip and the ds_write pass.
//   * 8 waves as 2(M) x 4(N), each 128x64 = 4x2 v_mfma_f32_32x32x16_bf16 tiles (128 acc VGPRs);
//   * BK = 64: A and W tiles are [256][128 B] row images, two buffers = 128 KiB LDS, 1 block/CU;
//   * a wave-instruction of global_load_lds writes 1 KiB = 8 rows x 128 B linearly, so the
//     bank-conflict swizzle (16-B chunk ^= (row>>1)&7) is applied to the per-lane SOURCE
//     address and again on the ds_read_b128 (both sides or neither);
//   * two main loops: the two-phase loop (issue tile t+1's DMA, MFMA tile t, vmcnt(0) + barrier;
//     192- or 256-row tiles) and the ping-pong loop for 256-row tiles (counted vmcnt, raw barriers;
//     see gemm256pp_kernel); gemm256_launch picks by the CU-rounds a shape wastes;
//   * tiles are walked in 8 x 4 patches per XCD (tile_coords256);
//   * compile-time epilogues through per-wave LDS slabs -> row-contiguous 16-B stores, branch-free
//     on interior tiles (epilogue256);
//   * the single-stream and ping-pong loops run on either MFMA shape (M16: v_mfma_f32_16x16x32, the
//     default, or v_mfma_f32_32x32x16; SKIMI_GEMM256_MFMA=16|32): the same cycles per FLOP, but on
//     random data the chip holds a higher clock on the 16x16 shape (profiles/r04_peaks.json).
#include <stdlib.h>

#include <type_traits>

#include "common.h"
#include "env.h"
#include "gemm_epilogue.h"
#include "gfx950.h"

namespace skimi {

// blockIdx -> output tile: XCD-contiguous tile ids (gfx950.h), ordered so that the ~32 tiles an XCD runs at once
// form an 8-row x 4-column patch
// (groups of 8 tile rows, column-major inside a group): per K-step that patch pulls 8 A panels and
// 4 W panels through the L2 instead of 2-3 A panels and every W panel (row-major order), which is
// what bounds the LDS-DMA stream.
__device__ __forceinline__ void tile_coords256(const GemmArgs& p, int& tm, int& tn) {
    const int id = xcd_contiguous_id(blockIdx.x, p.ntm * p.ntn);
    constexpr int GM = 8;
    const int per_group = GM * p.ntn;
    const int group = id / per_group, within = id - group * per_group;
    const int rows = min(GM, p.ntm - group * GM);
    tn = within / rows;
    tm = group * GM + within - tn * rows;
}

// Epilogue shared by both main loops: MT passes of 32 rows through this wave's private 8-KiB LDS
// slab -> row-contiguous 16-B (fp32) / 8-B (bf16) stores.  The caller guarantees that no wave
// still reads operand tiles from LDS (the slabs alias buffer 0).
//
// Stores share the vmcnt counter with loads on gfx9, and hipcc cannot count across branches: a
// per-row `if (m < M)` turns into s_cbranch_execz + s_waitcnt vmcnt(0) per row, i.e. every store
// waits for the previous one's round trip.  So the interior tiles (all but the last tile row /
// column) take a branch-free straight-line path, and only edge tiles run the checked loop.
//
// The residual epilogue (EPI 2) is a chain of global round trips per pass (residual load -> add ->
// store, and loads wait behind older stores in vmcnt), so the residual rows of the next PF passes
// are requested ahead: PF passes x 8 float4 = 32 PF registers.
// H16: the 16-bit rows of EPI 1 / 3 are fp16 instead of bf16 (compile time: a runtime select would double the
// conversions of an epilogue whose VALU time is exposed)
template <bool H16>
__device__ __forceinline__ bf16x4 pack4_16(float y0, float y1, float y2, float y3) {
    bf16x4 hb;
    if constexpr (H16) {
        hb[0] = (short)f2h(y0); hb[1] = (short)f2h(y1); hb[2] = (short)f2h(y2); hb[3] = (short)f2h(y3);
    } else {
        hb[0] = (short)f2bf(y0); hb[1] = (short)f2bf(y1); hb[2] = (short)f2bf(y2); hb[3] = (short)f2bf(y3);
    }
    return hb;
}

// Slab writers: pass i of a wave's (32 MT) x 64 accumulator strip -> its 32 x 64 fp32 slab (row-major, 64 columns).
// 32x32 tiles acc[i][j] (columns 32 j): lane l holds column l & 31, rows 8 (r >> 2) + 4 (l >> 5) + (r & 3)
template <int MT>
__device__ __forceinline__ void acc_to_slab(float* stg, const f32x16 (&acc)[MT][2], int i, int lane) {
    const int l31 = lane & 31, lh = lane >> 5;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) stg[((r & 3) + 8 * (r >> 2) + 4 * lh) * 64 + j * 32 + l31] = acc[i][j][r];
}
// 16x16 tiles acc[b][c] (rows 16 b, columns 16 c): lane l holds column l & 15, rows 4 (l >> 4) + r
template <int MT>
__device__ __forceinline__ void acc_to_slab(float* stg, const f32x4 (&acc)[2 * MT][4], int i, int lane) {
    const int l15 = lane & 15, lq = lane >> 4;
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int r = 0; r < 4; ++r) stg[(16 * b + 4 * lq + r) * 64 + 16 * c + l15] = acc[2 * i + b][c][r];
}

// ACC: f32x16[MT][2] (32x32 tiles) or f32x4[2 MT][4] (16x16 tiles); everything after the slab is layout-free
template <int MT, int EPI, int PF = 2, bool H16 = false, typename ACC>
__device__ __forceinline__ void epilogue256(const GemmArgs& p, ACC& acc, char* smem, int wave, int lane,
                                            int wr, int wc, int m0, int n0) {
    float* stg = reinterpret_cast<float*>(smem) + wave * (32 * 64);
    const int n = n0 + wc * 64 + 4 * (lane & 15);
    if (p.dbg & 8) {   // timing ablation: no epilogue (keeps the accumulators alive through one store)
        if (acc[0][0][0] == 123.456f) ((float*)p.out)[0] = acc[MT - 1][1][sizeof(acc[0][0]) / 4 - 1];
        return;
    }
    const bool interior = (m0 + 64 * MT <= p.M) && (n0 + 256 <= p.N) && !(p.dbg & 4);   // block-uniform
    float4 bs = make_float4(0, 0, 0, 0), gm = make_float4(1, 1, 1, 1);
    if (EPI != 0 && n < p.N) {
        if (p.bias) bs = *reinterpret_cast<const float4*>(p.bias + n);
        if (EPI == 2) gm = *reinterpret_cast<const float4*>(p.gamma + n);
    }
    // accumulators of row block i -> this wave's slab.  Same-wave LDS write -> read: DS ops of one
    // wave execute in order; the compiler only needs to keep them in program order.
#define SKIMI_ACC_TO_SLAB(i)                                                                                   \
    do {                                                                                                        \
        acc_to_slab<MT>(stg, acc, i, lane);                                                                     \
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");                                                  \
        wait_lgkmcnt0(); /* lgkmcnt(0) */                                                                       \
    } while (0)

    if (EPI == 2 && interior) {
        const int mrow0 = m0 + wr * (32 * MT) + (lane >> 4);
        float4 r[PF][8];
#pragma unroll
        for (int i = 0; i < PF && i < MT; ++i)
#pragma unroll
            for (int it = 0; it < 8; ++it)
                r[i][it] = *reinterpret_cast<const float4*>((const float*)p.resid + (long)(mrow0 + i * 32 + it * 4) * p.ldr + n);
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            SKIMI_ACC_TO_SLAB(i);
            const int mrow = mrow0 + i * 32;
            float4 v[8];
#pragma unroll
            for (int it = 0; it < 8; ++it)
                v[it] = *reinterpret_cast<const float4*>(&stg[(it * 4 + (lane >> 4)) * 64 + 4 * (lane & 15)]);
#pragma unroll
            for (int it = 0; it < 8; ++it) {
                const float4 rr = r[i % PF][it];
                f32x4 ov = {rr.x + gm.x * (v[it].x + bs.x), rr.y + gm.y * (v[it].y + bs.y),
                            rr.z + gm.z * (v[it].z + bs.z), rr.w + gm.w * (v[it].w + bs.w)};
                *reinterpret_cast<f32x4*>((float*)p.out + (long)(mrow + it * 4) * p.ldo + n) = ov;
            }
            if (i + PF < MT) {
#pragma unroll
                for (int it = 0; it < 8; ++it)
                    r[i % PF][it] =
                        *reinterpret_cast<const float4*>((const float*)p.resid + (long)(mrow + PF * 32 + it * 4) * p.ldr + n);
            }
            wait_lgkmcnt0();   // slab reads retired before the next pass overwrites it
        }
        return;
    }
    if (EPI != 0 && interior) {
        const bool mx = EPI == 3 && p.out_dtype == SKIMI_FP8MX;   // MXFP8 result: 8 lanes = one 32-column scale block of a row
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            SKIMI_ACC_TO_SLAB(i);
            const int mrow = m0 + wr * (32 * MT) + i * 32 + (lane >> 4);
            float4 v[8];
#pragma unroll
            for (int it = 0; it < 8; ++it)
                v[it] = *reinterpret_cast<const float4*>(&stg[(it * 4 + (lane >> 4)) * 64 + 4 * (lane & 15)]);
            unsigned sb_mine = 0;   // MXFP8: the scale of pass it = lane & 7, so that the 64 scale bytes of the slab go out in one store
#pragma unroll
            for (int it = 0; it < 8; ++it) {
                float y0 = v[it].x + bs.x, y1 = v[it].y + bs.y, y2 = v[it].z + bs.z, y3 = v[it].w + bs.w;
                if (EPI == 3) {
                    const f32x2_t g0 = gelu_erf2(f32x2_t{y0, y1}), g1 = gelu_erf2(f32x2_t{y2, y3});
                    y0 = g0.x; y1 = g0.y; y2 = g1.x; y3 = g1.y;
                }
                if (mx) {
                    const unsigned sb = mx_scale_byte(max8(fmaxf(fmaxf(fabsf(y0), fabsf(y1)), fmaxf(fabsf(y2), fabsf(y3)))));
                    const long row = mrow + it * 4;
                    *reinterpret_cast<int*>((unsigned char*)p.out + row * p.ldo + n) = mx_pack4(y0, y1, y2, y3, mx_inv_scale(sb));
                    sb_mine = (lane & 7) == it ? sb : sb_mine;
                    if (it == 7) p.out_scales[(long)(mrow + (lane & 7) * 4) * (p.N >> 5) + (n >> 5)] = (unsigned char)sb_mine;
                    continue;
                }
                *reinterpret_cast<bf16x4*>((unsigned short*)p.out + (long)(mrow + it * 4) * p.ldo + n) = pack4_16<H16>(y0, y1, y2, y3);
            }
            wait_lgkmcnt0();   // slab reads retired before the next pass overwrites it
        }
        return;
    }
#pragma unroll
    for (int i = 0; i < MT; ++i) {
        SKIMI_ACC_TO_SLAB(i);
        const int mrow = m0 + wr * (32 * MT) + i * 32 + (lane >> 4);
        if (EPI != 0) {
            // edge tiles: checked, rolled loop
#pragma unroll 1
            for (int it = 0; it < 8; ++it) {
                const int m = mrow + it * 4;
                if (m >= p.M || n >= p.N || (p.dbg & 4)) continue;
                const float4 v = *reinterpret_cast<const float4*>(&stg[(it * 4 + (lane >> 4)) * 64 + 4 * (lane & 15)]);
                float y0 = v.x + bs.x, y1 = v.y + bs.y, y2 = v.z + bs.z, y3 = v.w + bs.w;
                if (EPI == 2) {
                    const float4 r = *reinterpret_cast<const float4*>((const float*)p.resid + (long)m * p.ldr + n);
                    f32x4 ov = {r.x + gm.x * y0, r.y + gm.y * y1, r.z + gm.z * y2, r.w + gm.w * y3};
                    *reinterpret_cast<f32x4*>((float*)p.out + (long)m * p.ldo + n) = ov;
                } else {
                    if (EPI == 3) { y0 = gelu_erf(y0); y1 = gelu_erf(y1); y2 = gelu_erf(y2); y3 = gelu_erf(y3); }
                    if (EPI == 3 && p.out_dtype == SKIMI_FP8MX) {   // rows are valid or not per 16 lanes: the 8-lane groups are whole
                        const unsigned sb = mx_scale_byte(max8(fmaxf(fmaxf(fabsf(y0), fabsf(y1)), fmaxf(fabsf(y2), fabsf(y3)))));
                        *reinterpret_cast<int*>((unsigned char*)p.out + (long)m * p.ldo + n) = mx_pack4(y0, y1, y2, y3, mx_inv_scale(sb));
                        if ((lane & 7) == 0) p.out_scales[(long)m * (p.N >> 5) + (n >> 5)] = (unsigned char)sb;
                        continue;
                    }
                    *reinterpret_cast<bf16x4*>((unsigned short*)p.out + (long)m * p.ldo + n) = pack4_16<H16>(y0, y1, y2, y3);
                }
            }
        } else {
#pragma unroll 1
            for (int it = 0; it < 8; ++it) {
                const int m = mrow + it * 4;
                if (m >= p.M || n >= p.N) continue;
                const float4 v = *reinterpret_cast<const float4*>(&stg[(it * 4 + (lane >> 4)) * 64 + 4 * (lane & 15)]);
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
        }
        wait_lgkmcnt0();
    }
#undef SKIMI_ACC_TO_SLAB
}

// EPI: 0 = generic epilogue (runtime flags); 1 = bias -> bf16 rows (qkv); 3 = bias, GELU -> bf16
//      rows (fc1); 2 = bias, LayerScale, fp32 residual -> fp32 rows, plain row map (proj, fc2)
// F16 (all three loops): fp16 operands on v_mfma_f32_32x32x16_f16 (SKIMI_PREC_F16); EPI 3 then writes fp16 rows (the
// MLP's hidden activation, fc2's operand), EPI 1 still bf16 rows (qkv: the attention products stay bf16)
template <int MT, int EPI, bool F16 = false>   // M tiles of 32 rows per wave: BM = 64 * MT (192 or 256)
__global__ __launch_bounds__(512, 2) void gemm256_kernel(const GemmArgs p) {
    constexpr int BM = 64 * MT, BN = 256, BK = 64;
    constexpr int RB = 128;                    // LDS row bytes
    constexpr int A_TILE = BM * RB, W_TILE = BN * RB, BUF = A_TILE + W_TILE;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 2, wc = wave & 3;
    const int l31 = lane & 31, lh = lane >> 5;

    int tm, tn;
    tile_coords256(p, tm, tn);
    const int m0 = tm * BM, n0 = tn * BN;
    const int nkt = p.K / BK;
    if ((p.dbg & 16) && blockIdx.x < 256) {
        // experiment: de-phase the CUs so epilogue store bursts overlap other CUs' main loops
        const long long t0 = wall_clock64();
        const long long wait = (long long)((blockIdx.x >> 3) & 3) * (nkt * 50 + 300) / 4;
        while (wall_clock64() - t0 < wait) __builtin_amdgcn_s_sleep(32);
    }

    // staging: wave-instruction j of this wave covers tile rows 8*(4*wave + j) .. +7;
    // lane -> (row = lane>>3, LDS chunk = lane&7), source chunk = LDS chunk ^ ((row>>1)&7)
    const unsigned short* A = (const unsigned short*)p.A;
    const unsigned short* W = (const unsigned short*)p.W;
    const unsigned short* a_src[MT];
    const unsigned short* w_src[4];
#pragma unroll
    for (int j = 0; j < MT; ++j) {
        const int row = 8 * (MT * wave + j) + (lane >> 3);
        const int c = (lane & 7) ^ ((row >> 1) & 7);
        a_src[j] = A + (long)min(m0 + row, p.M - 1) * p.lda + c * 8;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int row = 8 * (4 * wave + j) + (lane >> 3);
        const int c = (lane & 7) ^ ((row >> 1) & 7);
        w_src[j] = W + (long)min(n0 + row, p.N - 1) * p.ldw + c * 8;
    }
    auto stage = [&](int buf, int kt) {
        char* ab = smem + buf * BUF + (MT * wave) * 8 * RB;
        char* wb = smem + buf * BUF + A_TILE + (4 * wave) * 8 * RB;
#pragma unroll
        for (int j = 0; j < MT; ++j)
            lds_dma16(a_src[j] + kt * BK, ab + j * 8 * RB);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            lds_dma16(w_src[j] + kt * BK, wb + j * 8 * RB);
    };

    f32x16 acc[MT][2];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    stage(0, 0);
    __syncthreads();   // hipcc drains the LDS-DMA (vmcnt(0)) ahead of the barrier
    for (int kt = 0; kt < nkt; ++kt) {
        const int cur = kt & 1;
        if (kt + 1 < nkt && !(p.dbg & 1)) stage(cur ^ 1, kt + 1);
        const char* ab = smem + cur * BUF;
        const char* wb = ab + A_TILE;
        // fragment reads are software-pipelined one k-step ahead of the MFMAs (two register sets,
        // pinned by sched_barrier): the ds_read latency of step s+1 hides under step s's 8 MFMAs
        bf16x8 af[2][MT], wf[2][2];
        auto load_frags = [&](int s, int set) {
#pragma unroll
            for (int i = 0; i < MT; ++i) {
                const int row = wr * (32 * MT) + i * 32 + l31;
                af[set][i] = *reinterpret_cast<const bf16x8*>(ab + row * RB + (((2 * s + lh) ^ ((row >> 1) & 7)) << 4));
            }
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int row = wc * 64 + j * 32 + l31;
                wf[set][j] = *reinterpret_cast<const bf16x8*>(wb + row * RB + (((2 * s + lh) ^ ((row >> 1) & 7)) << 4));
            }
        };
        if (!(p.dbg & 2)) {
        load_frags(0, 0);
        __builtin_amdgcn_sched_barrier(0);   // keep set 0's reads ahead of set 1's: counted lgkmcnt
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            if (s + 1 < 4) load_frags(s + 1, (s + 1) & 1);
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[i][j] = mfma_32x32x16<F16>(af[s & 1][i], wf[s & 1][j], acc[i][j]);
            __builtin_amdgcn_s_setprio(0);
            __builtin_amdgcn_sched_barrier(0);
        }
        }
        __syncthreads();
    }

    epilogue256<MT, EPI, 2, F16 && EPI == 3>(p, acc, smem, wave, lane, wr, wc, m0, n0);
}

// ---------------------------------------------------------------------------------------------
// Ping-pong main loop (256x256 tile only).  The two waves that share a SIMD (wr = 0 / wr = 1)
// run half a phase apart: while one issues its 8 MFMAs of a 64x32 output quadrant, the other
// reads the fragments of its next quadrant from LDS and issues its share of the LDS-DMA
// prefetch, then they swap at a raw s_barrier.  No vmcnt(0) and no fence inside the loop: the
// DMA of K-tile kt+2 is issued into the buffer of K-tile kt quarter by quarter, each quarter two
// or more barriers after its last reader, and retired by ONE counted s_waitcnt per K-tile.
//
// A K-tile (BK = 64) is staged as four 16-KiB quarter tiles, named by the phase that reads them:
//   HA[ih] : A rows 64*ih + {0..63} of both wave rows   (quadrants (ih, *))
//   HW[jh] : W rows 64*wc + 32*jh + {0..31}, wc = 0..3  (quadrants (*, jh))
// phase order (0,0) (0,1) (1,1) (1,0); fragment reads: P1 A[0] + W[0], P2 W[1], P3 A[1], P4 none
// (both W halves stay in registers).  DMA issue, two wave-instructions per wave and phase:
//   P1: HA[1](kt+1)   P2: HW[0](kt+1)   P3: HA[0](kt+2)   P4: HW[1](kt+2), then vmcnt(4):
// everything but the two quarters just issued has landed, i.e. all of K-tile kt+1.
// WAR distance: HA[0](kt) is last read in P1 and overwritten from P3 (4+ barriers later), HW[1]
// P2 -> P4, HA[1] P3 -> next P1, HW[0] P1 -> next P2.
// M16: a quadrant is 4 x 2 tiles of 16x16 in 2 k-steps of 32 (16 v_mfma_f32_16x16x32 instead of 8 of 32x32x16: the
// same MFMA cycles), with the same 8 + 4 fragment reads per phase (rows l & 15, 16-B chunk 4 s + (l >> 4)).

template <int EPI, int DEEP, bool F16 = false, bool M16 = false>
__global__ __launch_bounds__(512, 2) void gemm256pp_kernel(const GemmArgs p) {
    constexpr int MT = 4, BM = 256, BN = 256, BK = 64;
    constexpr int RB = 128;
    constexpr int A_TILE = BM * RB, W_TILE = BN * RB, BUF = A_TILE + W_TILE;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 2, wc = wave & 3;
    const int l31 = lane & 31, lh = lane >> 5;
    const int l15 = lane & 15, lq = lane >> 4;

    int tm, tn;
    tile_coords256(p, tm, tn);
    const int m0 = tm * BM, n0 = tn * BN;
    const int nkt = p.K / BK;

    // DMA pieces: quarter tile = 16 wave-instructions (8 rows x 128 B each); this wave issues
    // pieces g = 2*wave + j.  lane -> (row = lane>>3, LDS chunk = lane&7), source chunk swizzled.
    const unsigned short* A = (const unsigned short*)p.A;
    const unsigned short* W = (const unsigned short*)p.W;
    const unsigned short* a_src[2][2];   // [ih][j]
    const unsigned short* w_src[2][2];   // [jh][j]
    int a_row0[2][2], w_row0[2][2];      // wave-uniform first tile row of the piece
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int g = 2 * wave + j;
            a_row0[h][j] = (g >> 3) * 128 + 64 * h + 8 * (g & 7);
            w_row0[h][j] = (g >> 2) * 64 + 32 * h + 8 * (g & 3);
            int row = a_row0[h][j] + (lane >> 3);
            int c = (lane & 7) ^ ((row >> 1) & 7);
            a_src[h][j] = A + (long)min(((p.dbg & 64) ? 0 : m0) + row, p.M - 1) * p.lda + c * 8;
            row = w_row0[h][j] + (lane >> 3);
            c = (lane & 7) ^ ((row >> 1) & 7);
            w_src[h][j] = W + (long)min(((p.dbg & 64) ? 0 : n0) + row, p.N - 1) * p.ldw + c * 8;
        }
    const bool no_dma = p.dbg & 1, no_mfma = p.dbg & 2, no_rd = p.dbg & 32;
    auto issue_a = [&](int h, int kt) {
        if (no_dma) return;
        char* base = smem + (kt & 1) * BUF;
#pragma unroll
        for (int j = 0; j < 2; ++j)
            lds_dma16(a_src[h][j] + kt * BK, base + a_row0[h][j] * RB);
    };
    auto issue_w = [&](int h, int kt) {
        if (no_dma) return;
        char* base = smem + (kt & 1) * BUF + A_TILE;
#pragma unroll
        for (int j = 0; j < 2; ++j)
            lds_dma16(w_src[h][j] + kt * BK, base + w_row0[h][j] * RB);
    };

    f32x16 acc[MT][2];           // 32x32 tiles
    f32x4 acc16[2 * MT][4];      // M16: 16x16 tiles [16-row block][16-column block]
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
#pragma unroll
    for (int i = 0; i < 2 * MT; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc16[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    // prologue: all of K-tile 0, then the two quarters of K-tile 1 that the loop does not issue
    issue_a(0, 0); issue_w(0, 0); issue_w(1, 0); issue_a(1, 0);
    if (nkt > 1) {
        issue_a(0, 1);
        if (DEEP) issue_w(0, 1);
        issue_w(1, 1);
        if (DEEP) wait_vmcnt<6>(); else wait_vmcnt<4>();
    } else {
        wait_vmcnt<0>();
    }
    fenced_barrier();
    if (wr == 1) fenced_barrier();   // wave row 1 runs one barrier behind wave row 0

    bf16x8 af[2][4], wf[2][4];   // A: [row block within the quadrant][k-step]; W: [jh][k-step]
    bf16x8 af16[4][2], wf16[2][2][2];   // M16: A [16-row block][k-step]; W [jh][16-column block][k-step]
    if (no_rd) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int s = 0; s < 4; ++s) af[i][s] = wf[i][s] = af16[s][i] = wf16[i][s >> 1][s & 1] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
    }
    for (int kt = 0; kt < nkt; ++kt) {
        const char* ab = smem + (kt & 1) * BUF;
        const char* wb = ab + A_TILE;
        auto read_a = [&](int ih) {
            if (no_rd) return;
            if constexpr (M16) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int s = 0; s < 2; ++s) {
                        const int row = wr * 128 + ih * 64 + i * 16 + l15;
                        af16[i][s] = *reinterpret_cast<const bf16x8*>(ab + row * RB + (((4 * s + lq) ^ ((row >> 1) & 7)) << 4));
                    }
                return;
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const int row = wr * 128 + (2 * ih + i) * 32 + l31;
                    af[i][s] = *reinterpret_cast<const bf16x8*>(ab + row * RB + (((2 * s + lh) ^ ((row >> 1) & 7)) << 4));
                }
        };
        auto read_w = [&](int jh) {
            if (no_rd) return;
            if constexpr (M16) {
#pragma unroll
                for (int c = 0; c < 2; ++c)
#pragma unroll
                    for (int s = 0; s < 2; ++s) {
                        const int row = wc * 64 + jh * 32 + c * 16 + l15;
                        wf16[jh][c][s] = *reinterpret_cast<const bf16x8*>(wb + row * RB + (((4 * s + lq) ^ ((row >> 1) & 7)) << 4));
                    }
                return;
            }
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int row = wc * 64 + jh * 32 + l31;
                wf[jh][s] = *reinterpret_cast<const bf16x8*>(wb + row * RB + (((2 * s + lh) ^ ((row >> 1) & 7)) << 4));
            }
        };
#define SKIMI_QUADRANT(IH, JH)                                                                                  \
    do {                                                                                                         \
        fenced_barrier();                                                                                        \
        __builtin_amdgcn_s_setprio(1);                                                                           \
        if (no_mfma) {                                                                                           \
        } else if constexpr (M16) {                                                                              \
            _Pragma("unroll") for (int s = 0; s < 2; ++s) _Pragma("unroll") for (int i = 0; i < 4; ++i)          \
                _Pragma("unroll") for (int c = 0; c < 2; ++c) acc16[4 * IH + i][2 * JH + c] =                    \
                    mfma_16x16x32<F16>(af16[i][s], wf16[JH][c][s], acc16[4 * IH + i][2 * JH + c]);               \
        } else {                                                                                                 \
            _Pragma("unroll") for (int s = 0; s < 4; ++s) {                                                      \
                acc[2 * IH][JH] = mfma_32x32x16<F16>(af[0][s], wf[JH][s], acc[2 * IH][JH]);                       \
                acc[2 * IH + 1][JH] = mfma_32x32x16<F16>(af[1][s], wf[JH][s], acc[2 * IH + 1][JH]);               \
            }                                                                                                    \
        }                                                                                                        \
        __builtin_amdgcn_s_setprio(0);                                                                           \
        fenced_barrier();                                                                                        \
    } while (0)

        // P1
        read_w(0);
        read_a(0);
        if (kt + 1 < nkt) issue_a(1, kt + 1);
        SKIMI_QUADRANT(0, 0);
        // P2
        read_w(1);
        if (!DEEP && kt + 1 < nkt) issue_w(0, kt + 1);
        SKIMI_QUADRANT(0, 1);
        // P3
        read_a(1);
        if (kt + 2 < nkt) {
            issue_a(0, kt + 2);
            if (DEEP) issue_w(0, kt + 2);
        }
        SKIMI_QUADRANT(1, 1);
        // P4
        if (kt + 2 < nkt) {
            issue_w(1, kt + 2);
            if (DEEP) wait_vmcnt<6>(); else wait_vmcnt<4>();
        } else {
            wait_vmcnt<0>();
        }
        SKIMI_QUADRANT(1, 0);
#undef SKIMI_QUADRANT
    }
    if (wr == 0) fenced_barrier();   // re-align the two wave rows: nobody reads operand tiles any more

    if constexpr (M16) epilogue256<MT, EPI, 2, F16 && EPI == 3>(p, acc16, smem, wave, lane, wr, wc, m0, n0);
    else epilogue256<MT, EPI, 2, F16 && EPI == 3>(p, acc, smem, wave, lane, wr, wc, m0, n0);
}


// Single-stream loop: 4 waves (one per SIMD), each a 128x128 quadrant = 4x4 MFMA tiles (256
// accumulator registers; the kernel runs at one wave per SIMD, so 512 are there).  Every wave
// software-pipelines its own stream — the 8 fragment reads of k-step s+1 and its share of the
// LDS-DMA go out between the 16 MFMAs of k-step s — and there is ONE workgroup barrier per K-tile
// instead of eight hand-offs between two wave rows.  Fragment reads drop to 128 KiB per K-tile
// (8 per 16 MFMAs) from 192 KiB.
//
// LDS is a ring of ten 16-KiB slots (all 160 KiB); a K-tile is four pieces of 128 rows x 128 B:
// q = 0,1 the A rows of wave row 0 / 1, q = 2,3 the W rows of wave column 0 / 1; piece q of
// K-tile kt sits in slot (4 kt + q) mod 10.  The two spare slots let half of K-tile kt+2 go out a
// whole K-tile early:
//   k-step 1, 2 of kt : issue (kt+2; q = 0), (kt+2; q = 1)      -> the slots K-tile kt-1's W left
//   k-step 3 of kt    : lgkmcnt(0), vmcnt(8) = all of kt+1 landed, barrier (= K-tile kt released),
//                       read (kt+1, k-step 0), issue (kt+2; q = 2, 3) -> K-tile kt's A slots
// M16: the quadrant is 8 x 8 tiles of 16x16 (256 accumulator registers again) and a K-tile is 2 k-steps of 32, each
// with 8 + 8 fragment reads (rows l & 15, 16-B chunk 4 s + (l >> 4)) and 64 v_mfma_f32_16x16x32: the same reads, bytes
// and MFMA cycles per K-tile.  Each k-step stands for two of the 32x32x16 loop's, so the DMA and barrier plan keeps
// its meaning:
//   k-step 0 of kt    : read (kt, k-step 1), issue (kt+2; q = 0, 1)
//   k-step 1 of kt    : lgkmcnt(0), vmcnt(8), barrier, read (kt+1, k-step 0), issue (kt+2; q = 2, 3)
template <int EPI, bool F16 = false, bool M16 = false>
__global__ __launch_bounds__(256, 1) void gemm256w4_kernel(const GemmArgs p) {
    constexpr int RB = 128, BK = 64, PIECE = 128 * RB, NSLOT = 10;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1, wc = wave & 1;
    const int l31 = lane & 31, lh = lane >> 5;

    int tm, tn;
    tile_coords256(p, tm, tn);
    const int m0 = tm * 256, n0 = tn * 256;
    const int nkt = p.K / BK;
    // DMA: a piece is 16 wave-instructions (8 rows x 128 B each); this wave issues 4*wave + j
    const unsigned short* src[4][4];   // [q][j]
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int row = (4 * wave + j) * 8 + (lane >> 3);
            const int c = (lane & 7) ^ ((row >> 1) & 7);
            src[q][j] = q < 2 ? (const unsigned short*)p.A + (long)min(m0 + 128 * q + row, p.M - 1) * p.lda + c * 8
                              : (const unsigned short*)p.W + (long)min(n0 + 128 * (q - 2) + row, p.N - 1) * p.ldw + c * 8;
        }
    auto issue = [&](int q, int kt, int slot) {
        char* base = smem + slot * PIECE + (4 * wave) * 8 * RB;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            lds_dma16(src[q][j] + kt * BK, base + j * 8 * RB);
    };

    if constexpr (M16) {
    // fragment reads: 16-row block i of this wave's A piece (n = i) / W piece (n = 8 + i), k-step s
    const int l15 = lane & 15;
    const int t = (lane >> 4) ^ ((l15 >> 1) & 7);
    const int lane_off = l15 * RB;
    bf16x8 fa0[8], fb0[8], fa1[8], fb1[8];
    auto read_one = [&](int sb, int s, int n, bf16x8 (&fa)[8], bf16x8 (&fb)[8]) {
        int sa = sb + wr, sw = sb + 2 + wc;
        sa = sa >= NSLOT ? sa - NSLOT : sa;
        sw = sw >= NSLOT ? sw - NSLOT : sw;
        const int off = lane_off + (((4 * s) ^ t) << 4) + (n & 7) * 16 * RB;
        if (n < 8) fa[n] = *reinterpret_cast<const bf16x8*>(smem + sa * PIECE + off);
        else fb[n - 8] = *reinterpret_cast<const bf16x8*>(smem + sw * PIECE + off);
    };
    auto issue_one = [&](int q, int j, int kt, int slot) {
        lds_dma16(src[q][j] + kt * BK, smem + slot * PIECE + (4 * wave + j) * 8 * RB);
    };

    // [column half h][16-row block i][16-column block c]: columns 64 h + 16 c.  The MFMAs are inline asm on accumulators
    // pinned in AGPRs: with the builtin, hipcc shuttles ~590 of these 256 registers per K-tile through
    // v_accvgpr_mov / read / write.  hipcc pads nothing around an asm statement, so the wait states the MFMAs need are
    // written out: s_nop 1 between the accumulators' v_accvgpr_write and the first MFMA, 12 states between the last
    // MFMA and the epilogue's reads (8-pass XDL).
    f32x4 acc[2][8][4];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                acc[h][i][c] = f32x4{0.f, 0.f, 0.f, 0.f};
                asm volatile("" : "+a"(acc[h][i][c]));
            }
    asm volatile("s_nop 1");
    auto mfma = [&](f32x4& c, const bf16x8& a, const bf16x8& b) {
        if constexpr (F16) asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+a"(c) : "v"(a), "v"(b));
        else asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+a"(c) : "v"(a), "v"(b));
    };
    // one k-step: 64 MFMAs, extra(g) placed after MFMA g (source order = issue order: asm volatile + sched_barrier)
    auto kstep = [&](bf16x8 (&fa)[8], bf16x8 (&fb)[8], auto&& extra) {
#pragma unroll
        for (int j = 0; j < 8; ++j)
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                mfma(acc[j >> 2][i][j & 3], fa[i], fb[j]);
                extra(8 * j + i);
                __builtin_amdgcn_sched_barrier(0);
            }
    };

    // prologue: K-tiles 0 and 1 whole
#pragma unroll
    for (int q = 0; q < 4; ++q) issue(q, 0, q);
    if (nkt > 1) {
#pragma unroll
        for (int q = 0; q < 4; ++q) issue(q, 1, 4 + q);
        wait_vmcnt<16>();
    } else {
        wait_vmcnt<0>();
    }
    fenced_barrier();
    int sb = 0;   // slot of piece 0 of K-tile kt
#pragma unroll
    for (int n = 0; n < 16; ++n) read_one(sb, 0, n, fa0, fb0);
    // One k-step: lgkmcnt(0) in front (its fragments were requested a whole k-step ago); the next k-step's 16 fragment
    // reads go one behind each of the first 16 MFMAs, this k-step's 8 DMA issues one behind every second of the next 16
    // (an MFMA holds the SIMD for 16 cycles here instead of 32); the rest run back to back.
#define SKIMI_W4_HEAD()                       \
    do {                                      \
        wait_lgkmcnt0();                      \
        __builtin_amdgcn_sched_barrier(0);    \
    } while (0)
#define SKIMI_W4_KTILE(N1, N2)                                                                       \
    do {                                                                                             \
        int s8 = sb + 8, s9 = sb + 9, s1 = sb + 1, nsb = sb + 4;                                     \
        s8 = s8 >= NSLOT ? s8 - NSLOT : s8;                                                          \
        s9 = s9 >= NSLOT ? s9 - NSLOT : s9;                                                          \
        s1 = s1 >= NSLOT ? s1 - NSLOT : s1;                                                          \
        nsb = nsb >= NSLOT ? nsb - NSLOT : nsb;                                                      \
        /* k-step 0: read (kt, k-step 1), issue (kt+2; q = 0, 1) */                                  \
        SKIMI_W4_HEAD();                                                                             \
        kstep(fa0, fb0, [&](int g) {                                                                 \
            if (g < 16) read_one(sb, 1, g, fa1, fb1);                                                \
            else if (N2 && g < 32 && (g & 1)) {                                              \
                const int d = (g - 16) >> 1;                                                         \
                issue_one(d >> 2, d & 3, kt + 2, (d >> 2) ? s9 : s8);                                \
            }                                                                                        \
        });                                                                                          \
        /* k-step 1: vmcnt(8) = all of kt+1 landed, barrier (= K-tile kt released),                  \
           read (kt+1, k-step 0), issue (kt+2; q = 2, 3) into K-tile kt's A slots */                 \
        SKIMI_W4_HEAD();                                                                             \
        if (N1) {                                                                                    \
            if (N2) wait_vmcnt<8>(); else wait_vmcnt<0>();                                           \
            fenced_barrier();                                                                        \
        }                                                                                            \
        kstep(fa1, fb1, [&](int g) {                                                                 \
            if (N1 && g < 16) read_one(nsb, 0, g, fa0, fb0);                                         \
            else if (N2 && g < 32 && (g & 1)) {                                              \
                const int d = (g - 16) >> 1;                                                         \
                issue_one(2 + (d >> 2), d & 3, kt + 2, (d >> 2) ? s1 : sb);                          \
            }                                                                                        \
        });                                                                                          \
        sb = nsb;                                                                                    \
    } while (0)
    int kt = 0;
    for (; kt + 2 < nkt; ++kt) SKIMI_W4_KTILE(true, true);
    if (kt + 1 < nkt) {
        SKIMI_W4_KTILE(true, false);
        ++kt;
    }
    SKIMI_W4_KTILE(false, false);
#undef SKIMI_W4_KTILE
#undef SKIMI_W4_HEAD
    // 12 states: last MFMA's D -> the epilogue's v_accvgpr_read; the pins make every accumulator a value of THIS point,
    // so that hipcc reads none of them out between the MFMAs
    asm volatile("s_nop 7\n\ts_nop 4");
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int c = 0; c < 4; ++c) asm volatile("" : "+a"(acc[h][i][c]));
    wait_lgkmcnt0();
    fenced_barrier();   // nobody reads operand pieces any more: the epilogue slabs alias slots 0 and 1

    epilogue256<4, EPI, 4, F16 && EPI == 3>(p, acc[0], smem, wave, lane, wr, 2 * wc, m0, n0);
    epilogue256<4, EPI, 4, F16 && EPI == 3>(p, acc[1], smem, wave, lane, wr, 2 * wc + 1, m0, n0);
    } else {
    // fragment reads: row block i of this wave's A piece / W piece, k-step s
    const int t = lh ^ ((l31 >> 1) & 7);
    const int lane_off = l31 * RB;
    bf16x8 fa0[4], fb0[4], fa1[4], fb1[4];
    auto read = [&](int sb, int s, bf16x8 (&fa)[4], bf16x8 (&fb)[4]) {
        int sa = sb + wr, sw = sb + 2 + wc;
        sa = sa >= NSLOT ? sa - NSLOT : sa;
        sw = sw >= NSLOT ? sw - NSLOT : sw;
        const char* pa = smem + sa * PIECE + lane_off + (((2 * s) ^ t) << 4);
        const char* pw = smem + sw * PIECE + lane_off + (((2 * s) ^ t) << 4);
#pragma unroll
        for (int i = 0; i < 4; ++i) fa[i] = *reinterpret_cast<const bf16x8*>(pa + i * 32 * RB);
#pragma unroll
        for (int i = 0; i < 4; ++i) fb[i] = *reinterpret_cast<const bf16x8*>(pw + i * 32 * RB);
    };

    f32x16 acc[2][4][2];   // [column half h][row block i][column block j]: columns 64 h + 32 j
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[h][i][j][r] = 0.f;
#define SKIMI_W4_MFMA(FA, FB)                                                                                   \
    _Pragma("unroll") for (int j = 0; j < 4; ++j) _Pragma("unroll") for (int i = 0; i < 4; ++i)                 \
        acc[j >> 1][i][j & 1] = mfma_32x32x16<F16>(FA[i], FB[j], acc[j >> 1][i][j & 1])

    // prologue: K-tiles 0 and 1 whole
#pragma unroll
    for (int q = 0; q < 4; ++q) issue(q, 0, q);
    if (nkt > 1) {
#pragma unroll
        for (int q = 0; q < 4; ++q) issue(q, 1, 4 + q);
        wait_vmcnt<16>();
    } else {
        wait_vmcnt<0>();
    }
    fenced_barrier();
    int sb = 0;   // slot of piece 0 of K-tile kt
    read(sb, 0, fa0, fb0);
    // One k-step: the fragments it multiplies were requested a whole k-step ago, so the lgkmcnt(0)
    // in front is free; then the next k-step's 8 fragment reads and this k-step's DMA issues are
    // dealt out between the first MFMAs (2 reads or 1 DMA per MFMA), the rest run back to back.
#define SKIMI_W4_HEAD()                       \
    do {                                      \
        wait_lgkmcnt0();                      \
        __builtin_amdgcn_sched_barrier(0);    \
    } while (0)
#define SKIMI_W4_TAIL(NDMA)                                                        \
    do {                                                                           \
        _Pragma("unroll") for (int g = 0; g < 4; ++g) {                            \
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                     \
            __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);                     \
        }                                                                          \
        _Pragma("unroll") for (int g = 0; g < NDMA; ++g) {                         \
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                     \
            __builtin_amdgcn_sched_group_barrier(0x010, 1, 0);                     \
        }                                                                          \
        __builtin_amdgcn_sched_group_barrier(0x008, 12 - NDMA, 0);                 \
        __builtin_amdgcn_sched_barrier(0);                                         \
    } while (0)
    // one K-tile; N1 / N2: K-tiles kt+1 / kt+2 exist (literals: the main loop runs with both, the
    // last two K-tiles are peeled so that the loop body is one straight-line scheduling region)
#define SKIMI_W4_KTILE(N1, N2)                                                      \
    do {                                                                            \
        int s8 = sb + 8, s9 = sb + 9, s1 = sb + 1, nsb = sb + 4;                    \
        s8 = s8 >= NSLOT ? s8 - NSLOT : s8;                                         \
        s9 = s9 >= NSLOT ? s9 - NSLOT : s9;                                         \
        s1 = s1 >= NSLOT ? s1 - NSLOT : s1;                                         \
        nsb = nsb >= NSLOT ? nsb - NSLOT : nsb;                                     \
        /* k-step 0 */                                                              \
        SKIMI_W4_HEAD();                                                            \
        read(sb, 1, fa1, fb1);                                                      \
        SKIMI_W4_MFMA(fa0, fb0);                                                    \
        SKIMI_W4_TAIL(0);                                                           \
        /* k-step 1 */                                                              \
        SKIMI_W4_HEAD();                                                            \
        read(sb, 2, fa0, fb0);                                                      \
        if (N2) issue(0, kt + 2, s8);                                               \
        SKIMI_W4_MFMA(fa1, fb1);                                                    \
        SKIMI_W4_TAIL((N2 ? 4 : 0));                                                \
        /* k-step 2 */                                                              \
        SKIMI_W4_HEAD();                                                            \
        read(sb, 3, fa1, fb1);                                                      \
        if (N2) issue(1, kt + 2, s9);                                               \
        SKIMI_W4_MFMA(fa0, fb0);                                                    \
        SKIMI_W4_TAIL((N2 ? 4 : 0));                                                \
        /* k-step 3 */                                                              \
        SKIMI_W4_HEAD();                                                            \
        if (N1) {                                                                   \
            if (N2) wait_vmcnt<8>(); else wait_vmcnt<0>();                          \
            fenced_barrier();                                                       \
            read(nsb, 0, fa0, fb0);                                                 \
            if (N2) {                                                               \
                issue(2, kt + 2, sb);                                               \
                issue(3, kt + 2, s1);                                               \
            }                                                                       \
        }                                                                           \
        SKIMI_W4_MFMA(fa1, fb1);                                                    \
        if (N1) SKIMI_W4_TAIL((N2 ? 8 : 0)); else __builtin_amdgcn_sched_barrier(0); \
        sb = nsb;                                                                   \
    } while (0)
    int kt = 0;
    for (; kt + 2 < nkt; ++kt) SKIMI_W4_KTILE(true, true);
    if (kt + 1 < nkt) {
        SKIMI_W4_KTILE(true, false);
        ++kt;
    }
    SKIMI_W4_KTILE(false, false);
#undef SKIMI_W4_KTILE
#undef SKIMI_W4_HEAD
#undef SKIMI_W4_TAIL
#undef SKIMI_W4_MFMA
    wait_lgkmcnt0();
    fenced_barrier();   // nobody reads operand pieces any more: the epilogue slabs alias slots 0 and 1

    epilogue256<4, EPI, 4, F16 && EPI == 3>(p, acc[0], smem, wave, lane, wr, 2 * wc, m0, n0);
    epilogue256<4, EPI, 4, F16 && EPI == 3>(p, acc[1], smem, wave, lane, wr, 2 * wc + 1, m0, n0);
    }
}


// ---------------------------------------------------------------------------------------------------------
// MXFP8 on the same single-stream loop (BASELINE config 5).  A K-tile is again 128 bytes per row -- now 128 e4m3
// elements -- so tile geometry, LDS ring, LDS-DMA and fragment addresses are gemm256w4_kernel's unchanged; what
// changes is the matrix instruction: one v_mfma_scale_f32_32x32x64_f8f6f4 (64 cycles) consumes the fragments of TWO
// bf16 k-steps, because its operand image (a lane's first 16 bytes = elements 16 lh .. of scale block 0, the next 16
// = of scale block 1; gemm_fp8.hip) is exactly chunk (4 ks + lh) followed by chunk (4 ks + 2 + lh), i.e. the bf16
// kernel's reads of k-steps 2 ks and 2 ks + 1.  So a K-tile is two fp8 k-steps of 16 MFMAs each, every one with 16
// fragment reads (the next k-step's) and up to 16 vector-memory instructions (LDS-DMA of K-tile kt + 2, the E8M0
// dwords of K-tile kt + 1 read straight from L2) dealt between its MFMAs: the same bytes per K-tile as the bf16
// loop, the same MFMA cycles, twice the K.  The E8M0 byte of (row, scale block 2 ks + lh) is picked by a per-lane
// shift (8 lh) and the instruction's op_sel (0 / 2).  Epilogues: epilogue256 (same accumulator layout).
typedef __attribute__((ext_vector_type(8))) int i32x8_t;
typedef __attribute__((ext_vector_type(4))) int i32x4_t;

template <int EPI>
__global__ __launch_bounds__(256, 1) void gemm256w4_fp8_kernel(const GemmArgs p) {
    constexpr int RB = 128, BK = 128, PIECE = 128 * RB, NSLOT = 10;   // BK in bytes = elements
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1, wc = wave & 1;
    const int l31 = lane & 31, lh = lane >> 5;

    int tm, tn;
    tile_coords256(p, tm, tn);
    const int m0 = tm * 256, n0 = tn * 256;
    const int nkt = p.K / BK;
    const unsigned char* src[4][4];   // [q][j]
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int row = (4 * wave + j) * 8 + (lane >> 3);
            const int c = (lane & 7) ^ ((row >> 1) & 7);
            src[q][j] = q < 2 ? (const unsigned char*)p.A + (long)min(m0 + 128 * q + row, p.M - 1) * p.lda + c * 16
                              : (const unsigned char*)p.W + (long)min(n0 + 128 * (q - 2) + row, p.N - 1) * p.ldw + c * 16;
        }
    auto issue = [&](int q, int kt, int slot) {
        char* base = smem + slot * PIECE + (4 * wave) * 8 * RB;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            lds_dma16(src[q][j] + (long)kt * BK, base + j * 8 * RB);
    };
    // E8M0 dwords (4 scale blocks of a K-tile) of this lane's rows: A rows 128 wr + 32 i + l31, W rows 128 wc + 32 j + l31
    const unsigned* asc[4];
    const unsigned* wsc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        asc[i] = reinterpret_cast<const unsigned*>(p.a_scales + (long)min(m0 + 128 * wr + 32 * i + l31, p.M - 1) * p.lsa);
        wsc[i] = reinterpret_cast<const unsigned*>(p.w_scales + (long)min(n0 + 128 * wc + 32 * i + l31, p.N - 1) * p.lsw);
    }
    unsigned sa[4], sw[4], san[4], swn[4];
    auto load_scales = [&](int kt) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            san[i] = asc[i][kt];
            swn[i] = wsc[i][kt];
        }
    };
    auto take_scales = [&]() {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            sa[i] = san[i] >> (8 * lh);
            sw[i] = swn[i] >> (8 * lh);
        }
    };

    // fragment reads of one fp8 k-step = the bf16 kernel's reads of k-steps 2 ks and 2 ks + 1
    const int t = lh ^ ((l31 >> 1) & 7);
    const int lane_off = l31 * RB;
    i32x4_t fa0[2][4], fb0[2][4], fa1[2][4], fb1[2][4];
    auto readp = [&](int sb, int ks, i32x4_t (&fa)[2][4], i32x4_t (&fb)[2][4]) {
        int sA = sb + wr, sW = sb + 2 + wc;
        sA = sA >= NSLOT ? sA - NSLOT : sA;
        sW = sW >= NSLOT ? sW - NSLOT : sW;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int s = 2 * ks + h;
            const char* pa = smem + sA * PIECE + lane_off + (((2 * s) ^ t) << 4);
            const char* pw = smem + sW * PIECE + lane_off + (((2 * s) ^ t) << 4);
#pragma unroll
            for (int i = 0; i < 4; ++i) fa[h][i] = *reinterpret_cast<const i32x4_t*>(pa + i * 32 * RB);
#pragma unroll
            for (int i = 0; i < 4; ++i) fb[h][i] = *reinterpret_cast<const i32x4_t*>(pw + i * 32 * RB);
        }
    };

    f32x16 acc[2][4][2];   // [column half h][row block i][column block j]: columns 64 h + 32 j
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[h][i][j][r] = 0.f;
#define SKIMI_F8_CAT(F, I) i32x8_t{F[0][I][0], F[0][I][1], F[0][I][2], F[0][I][3], F[1][I][0], F[1][I][1], F[1][I][2], F[1][I][3]}
#define SKIMI_F8_MFMA(FA, FB, OPSEL)                                                                             \
    _Pragma("unroll") for (int j = 0; j < 4; ++j) _Pragma("unroll") for (int i = 0; i < 4; ++i)                  \
        acc[j >> 1][i][j & 1] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(                                 \
            SKIMI_F8_CAT(FA, i), SKIMI_F8_CAT(FB, j), acc[j >> 1][i][j & 1], 0, 0, OPSEL, (int)sa[i], OPSEL, (int)sw[j])

    // prologue: the scales of K-tile 0, then K-tiles 0 and 1 whole
    load_scales(0);
#pragma unroll
    for (int q = 0; q < 4; ++q) issue(q, 0, q);
    if (nkt > 1) {
#pragma unroll
        for (int q = 0; q < 4; ++q) issue(q, 1, 4 + q);
        wait_vmcnt<16>();
    } else {
        wait_vmcnt<0>();
    }
    take_scales();
    fenced_barrier();
    int sb = 0;   // slot of piece 0 of K-tile kt
    readp(sb, 0, fa0, fb0);
#define SKIMI_F8_HEAD()                       \
    do {                                      \
        wait_lgkmcnt0();                      \
        __builtin_amdgcn_sched_barrier(0);    \
    } while (0)
    // 16 MFMAs with the next k-step's 16 fragment reads (2 per MFMA) and NV vector-memory instructions behind them
#define SKIMI_F8_TAIL(NV)                                                          \
    do {                                                                           \
        _Pragma("unroll") for (int g = 0; g < 8; ++g) {                            \
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                     \
            __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);                     \
        }                                                                          \
        _Pragma("unroll") for (int g = 0; g < 8; ++g) {                            \
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                     \
            if (NV > 0) __builtin_amdgcn_sched_group_barrier(0x010, (NV + 7) / 8, 0); \
        }                                                                          \
        __builtin_amdgcn_sched_barrier(0);                                         \
    } while (0)
    // one K-tile; N1 / N2: K-tiles kt+1 / kt+2 exist; PW: vmcnt that leaves only what was issued AFTER this tile's scales
#define SKIMI_F8_KTILE(N1, N2, PW)                                                  \
    do {                                                                            \
        int s8 = sb + 8, s9 = sb + 9, s1 = sb + 1, nsb = sb + 4;                    \
        s8 = s8 >= NSLOT ? s8 - NSLOT : s8;                                         \
        s9 = s9 >= NSLOT ? s9 - NSLOT : s9;                                         \
        s1 = s1 >= NSLOT ? s1 - NSLOT : s1;                                         \
        nsb = nsb >= NSLOT ? nsb - NSLOT : nsb;                                     \
        /* k-step 0: scale blocks 0 / 1 */                                          \
        SKIMI_F8_HEAD();                                                            \
        readp(sb, 1, fa1, fb1);                                                     \
        if (N2) {                                                                   \
            issue(0, kt + 2, s8);                                                   \
            issue(1, kt + 2, s9);                                                   \
        }                                                                           \
        SKIMI_F8_MFMA(fa0, fb0, 0);                                                 \
        SKIMI_F8_TAIL((N2 ? 8 : 0));                                                \
        /* k-step 1: scale blocks 2 / 3 */                                          \
        SKIMI_F8_HEAD();                                                            \
        if (N1) {                                                                   \
            if (N2) wait_vmcnt<8>(); else wait_vmcnt<0>();                          \
            fenced_barrier();                                                       \
            readp(nsb, 0, fa0, fb0);                                                \
            load_scales(kt + 1);                                                    \
            if (N2) {                                                               \
                issue(2, kt + 2, sb);                                               \
                issue(3, kt + 2, s1);                                               \
            }                                                                       \
        }                                                                           \
        SKIMI_F8_MFMA(fa1, fb1, 2);                                                 \
        if (N1) SKIMI_F8_TAIL((N2 ? 16 : 8)); else __builtin_amdgcn_sched_barrier(0); \
        if (N1) {                                                                   \
            wait_vmcnt<PW>();   /* the scales of K-tile kt + 1 have landed */        \
            take_scales();                                                          \
        }                                                                           \
        sb = nsb;                                                                   \
    } while (0)
    int kt = 0;
    for (; kt + 2 < nkt; ++kt) SKIMI_F8_KTILE(true, true, 8);
    if (kt + 1 < nkt) {
        SKIMI_F8_KTILE(true, false, 0);
        ++kt;
    }
    SKIMI_F8_KTILE(false, false, 0);
#undef SKIMI_F8_KTILE
#undef SKIMI_F8_HEAD
#undef SKIMI_F8_TAIL
#undef SKIMI_F8_MFMA
#undef SKIMI_F8_CAT
    wait_lgkmcnt0();
    fenced_barrier();   // nobody reads operand pieces any more: the epilogue slabs alias slots 0 and 1

    epilogue256<4, EPI, 4>(p, acc[0], smem, wave, lane, wr, 2 * wc, m0, n0);
    epilogue256<4, EPI, 4>(p, acc[1], smem, wave, lane, wr, 2 * wc + 1, m0, n0);
}

// which compile-time epilogue serves this launch (0 = generic)
static int epi_kind(const GemmArgs& a) {
    const bool plain = a.vec4 && a.store_mode == 0 && a.out_rpb == 0 && a.out_off == 0 && a.out2 == nullptr &&
                       a.resid2 == nullptr && a.post_act == SKIMI_ACT_NONE && a.N % 4 == 0;
    if (!plain) return 0;
    if (a.gamma == nullptr && a.resid == nullptr && (a.out_dtype == SKIMI_BF16 || a.out_dtype == SKIMI_F16)) {
        // the 16-bit format a compile-time epilogue writes is fixed by the kernel: bf16, except EPI 3 of the fp16 loops
        if (a.act == SKIMI_ACT_NONE && a.out_dtype == SKIMI_BF16) return 1;
        if (a.act == SKIMI_ACT_GELU && a.out_dtype == (a.f16 ? SKIMI_F16 : SKIMI_BF16)) return 3;
        return 0;
    }
    if (a.out_dtype == SKIMI_FP8MX && a.out_scales != nullptr && a.gamma == nullptr && a.resid == nullptr && a.bias != nullptr &&
        a.act == SKIMI_ACT_GELU && a.N % 128 == 0)
        return 3;   // MXFP8 result (gemm256w4_fp8_kernel only)
    if (a.out_dtype == SKIMI_F32 && a.gamma != nullptr && a.resid != nullptr && a.resid_dtype == SKIMI_F32 &&
        a.resid_rpb == 0 && a.resid_off == 0 && a.act == SKIMI_ACT_NONE)
        return 2;
    return 0;
}

bool gemm256_eligible(const skimi_gemm_desc* d) {
    const bool bf = d->prec == SKIMI_PREC_BF16 && d->a_dtype == SKIMI_BF16 && d->w_dtype == SKIMI_BF16;
    const bool hf = d->prec == SKIMI_PREC_F16 && d->a_dtype == SKIMI_F16 && d->w_dtype == SKIMI_F16;
    return (bf || hf) && d->a_mode == 0 &&
           d->store_mode == 0 && d->K % 64 == 0 && d->lda % 8 == 0 && d->ldw % 8 == 0 && d->M >= 2048 &&
           d->N >= 512 && (((uintptr_t)d->A | (uintptr_t)d->W) & 15) == 0;
}

// calls f with the launch's epilogue kind as a compile-time constant: f(std::integral_constant<int, EPI>)
template <typename F>
static int dispatch_epi(int epi, F&& f) {
    if (epi == 1) return f(std::integral_constant<int, 1>{});
    if (epi == 2) return f(std::integral_constant<int, 2>{});
    if (epi == 3) return f(std::integral_constant<int, 3>{});
    return f(std::integral_constant<int, 0>{});
}

// the two-phase loop on tiles of 64 * MT rows
template <int MT, bool F16>
static int launch256(GemmArgs& a, hipStream_t st, int epi) {
    return dispatch_epi(epi, [&](auto e) {
        return launch_tiles<gemm256_kernel<MT, decltype(e)::value, F16>>(a, st, 2ull * (64 * MT + 256) * 128, 512, cdiv(a.M, 64 * MT),
                                                                         cdiv(a.N, 256), "gemm256");
    });
}

// the single-stream (w4) or the ping-pong loop on 256-row tiles
template <bool F16, bool M16>
static int gemm256_pick_loop(GemmArgs& a, hipStream_t st, int epi, bool w4) {
    const int64_t ntm = cdiv(a.M, 256), ntn = cdiv(a.N, 256);
    if (w4) {
        return dispatch_epi(epi, [&](auto e) {
            return launch_tiles<gemm256w4_kernel<decltype(e)::value, F16, M16>>(a, st, 10ull * 128 * 128, 256, ntm, ntn, "gemm256w4");
        });
    }
    return dispatch_epi(epi, [&](auto e) {
        constexpr int EPI = decltype(e)::value;
        constexpr size_t lds = 2ull * (256 + 256) * 128;
        if constexpr (F16) return launch_tiles<gemm256pp_kernel<EPI, 1, true, M16>>(a, st, lds, 512, ntm, ntn, "gemm256pp");
        const int deep = (int)env_switch("SKIMI_GEMM256_DEEP", 1);
        return deep ? launch_tiles<gemm256pp_kernel<EPI, 1, false, M16>>(a, st, lds, 512, ntm, ntn, "gemm256pp")
                    : launch_tiles<gemm256pp_kernel<EPI, 0, false, M16>>(a, st, lds, 512, ntm, ntn, "gemm256pp");
    });
}

template <bool F16>
static int gemm256_pick(GemmArgs& a, hipStream_t st, int epi, bool mt3, bool w4, int use_pp, bool m16) {
    if (mt3) return launch256<3, F16>(a, st, epi);
    // the fp16 build carries the two loops the dispatch picks (single-stream, ping-pong) + the 192-row one
    if (w4 || use_pp || F16) return m16 ? gemm256_pick_loop<F16, true>(a, st, epi, w4) : gemm256_pick_loop<F16, false>(a, st, epi, w4);
    if constexpr (!F16) return launch256<4, false>(a, st, epi);
    return SKIMI_ERR_ARG;
}

// pick the tile height (192 or 256 rows) that wastes the fewest CU-rounds for this shape:
// one workgroup per CU, so time ~ ceil(tiles / 256) * (rows per tile)
int gemm256_launch(GemmArgs& a, hipStream_t st) {
#ifdef SKIMI_ABLATIONS   // timing ablations (wrong results): only in a -DSKIMI_ABLATIONS build
    a.dbg = (int)env_switch("SKIMI_GEMM256_ABL", 0);
#else
    a.dbg = 0;
#endif
    auto cost = [&](int bm) {
        const long tiles = cdiv(a.M, bm) * cdiv(a.N, 256);
        return (double)cdiv(tiles, 256) * bm;
    };
    const int epi = epi_kind(a);
    // Which loop (measured on the aggregator shapes, M = 43968, interleaved A/B on one box):
    //   * 192-row tiles on the two-phase loop only when they save a whole lot of CU-rounds: at equal
    //     or slightly worse round counts the 256-row loops win (qkv: 301 us vs 267-281);
    //   * single-stream loop (4 waves) where the main loop dominates (qkv, fc2: -2..-6 %); ping-pong
    //     loop (8 waves) where the epilogue does (K <= 1024 with the residual epilogue, or GELU: its
    //     chain of LDS / VALU / global round trips runs on twice the waves there).
    // SKIMI_GEMM256_MT3 / _W4 / _PP = 0 / 1 force a choice (A/B timing).
    // MFMA shape of the single-stream and ping-pong loops (SKIMI_GEMM256_MFMA = 16 | 32): v_mfma_f32_16x16x32 by
    // default, measured against 32x32x16 interleaved on one box
    const bool m16 = (int)env_switch("SKIMI_GEMM256_MFMA", 16) != 32;
    const int use_pp = (int)env_switch("SKIMI_GEMM256_PP", 1);
    const int use_mt3 = (int)env_switch("SKIMI_GEMM256_MT3", -1);
    const int use_w4 = (int)env_switch("SKIMI_GEMM256_W4", -1);
    const bool mt3 = use_mt3 == 1 || (use_mt3 < 0 && cost(192) < 0.8 * cost(256));
    const bool w4 = use_w4 >= 0 ? use_w4 != 0 : (epi == 1 || (epi == 2 && a.K > 1024));
    // the loop gemm256_pick takes (the fp16 build has no two-phase 256-row loop: ping-pong in its place)
    const int loop = mt3 ? 2 : w4 ? 4 : (use_pp || a.f16) ? 3 : 1;
    set_gemm_path(SKIMI_GEMM_PATH_GEMM256, loop, (loop >= 3 && m16) ? 1 : 2, epi, 1);
    return a.f16 ? gemm256_pick<true>(a, st, epi, mt3, w4, use_pp, m16) : gemm256_pick<false>(a, st, epi, mt3, w4, use_pp, m16);
}

// MXFP8 operands on the single-stream 256 x 256 loop.  The caller (gemm_fp8_launch) has checked the shape: K = Kp
// (bytes per row, a multiple of 128), 16-byte aligned operands, one of the three compile-time epilogues.
int gemm256_fp8_launch(GemmArgs& a, hipStream_t st) {
    a.dbg = 0;
    return dispatch_epi(epi_kind(a), [&](auto e) {
        if constexpr (decltype(e)::value == 0) {
            set_error("gemm256_fp8: epilogue not supported");
            return SKIMI_ERR_ARG;
        } else {
            return launch_tiles<gemm256w4_fp8_kernel<decltype(e)::value>>(a, st, 10ull * 128 * 128, 256, cdiv(a.M, 256), cdiv(a.N, 256),
                                                                          "gemm256w4_fp8");
        }
    });
}

}  // namespace skimi
