// bf16 flash attention for head_dim 64 on gfx950 MFMA (v_mfma_f32_32x32x16_bf16), fp32 softmax:
// frame attention (batch = S frames, seq 1374) and global attention (batch = B, seq = S*1374) of
// vggt/vggt/models/aggregator.py:260-305 via F.scaled_dot_product_attention
// (vggt/vggt/layers/attention.py:60-61), and the 24 DINOv2 blocks.
//
// This file: the FIRST kernel, kept for A/B timing (SKIMI_ATTN_Q64=0; the 64-query-per-wave kernel of attention_q64.hip
// is the default), and that kernel's launcher, nothing else: what runs is decided in attention.hip (plan_attention).
// per workgroup 4 waves x 32 queries; K/V tiles of 64 keys double-buffered in LDS by LDS-DMA, one
// barrier per tile, row sums on the matrix pipe (ones-operand MFMAs).
// Products are "swapped" so each softmax row is lane-local:
//   S^T[key, q] = K Q^T   A = K from LDS (ds_read_b128, XOR-swizzled rows), B = Q from registers
//   O^T[d, q]  += V^T P^T A = V^T from LDS via ds_read_b64_tr_b16 (hardware transpose of a
//                          row-major [key][d] tile), B = P: the S^T accumulator converted to bf16
//                          in place (k order inside a step: key = 16s + 8(j>>2) + 4h + (j&3)).
// blockIdx -> (batch, head, q-block) is XCD-contiguous (gfx950.h) so one XCD's L2 holds a head's K/V.
#include <stdlib.h>

#include "attention_tile.h"
#include "common.h"
#include "kernels.h"

namespace skimi {

using namespace att;   // the K / V tile layout shared with attention_q64.hip and attention_x3.hip


__device__ __forceinline__ bf16x8 pack8(const f32x16& p, int s) {
    bf16x8 r;
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = (short)f2bf(p[8 * s + j]);
    return r;
}

template <int dbg>   // dbg != 0: timing ablations only (SKIMI_ATTN_ABL), results are wrong
__global__ __launch_bounds__(256, 4) void attn_bf16_kernel(const AttnArgs a, int nqb) {
    __shared__ __attribute__((aligned(16))) char smem[4 * TILE];   // [buf][K|V]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, lh = lane >> 5;

    const int id = xcd_contiguous_id();   // one XCD's L2 holds a head's K/V
    const int qb = id % nqb;
    const int bh = id / nqb;
    const int head = bh % a.heads, b = bh / a.heads;
    const int q0 = qb * 128 + wave * 32;

    const unsigned short* Q = (const unsigned short*)a.q + (long)b * a.q_batch + (long)head * a.q_head;
    const unsigned short* K = (const unsigned short*)a.k + (long)b * a.k_batch + (long)head * a.k_head;
    const unsigned short* V = (const unsigned short*)a.v + (long)b * a.v_batch + (long)head * a.v_head;
    unsigned short* O = (unsigned short*)a.out + (long)b * a.o_batch + (long)head * a.o_head;

    // Q fragments (B operand): lane (q, h) holds Q[q][16s + 8h + j]
    bf16x8 qf[4];
    {
        const int q = min(q0 + l31, a.seq_q - 1);
        const unsigned short* qp = Q + (long)q * a.q_row + 8 * lh;
#pragma unroll
        for (int s = 0; s < 4; ++s) qf[s] = *reinterpret_cast<const bf16x8*>(qp + 16 * s);
    }

    // K/V staging by LDS-DMA (global_load_lds_dwordx4), bank swizzles on the per-lane SOURCE chunk: attention_tile.h.
    // Rows past the end are clamped to the last valid row (finite data; their scores are masked
    // to -inf, so their P is exactly 0).  No staging registers, no ds_write pass.
    const int nkt = (a.seq_k + KV - 1) / KV;
    const bool ragged = (a.seq_k & (KV - 1)) != 0;
    const int srow = lane >> 3, sch = lane & 7;
    auto issue = [&](int buf, int kt) {
        char* kb = smem + buf * 2 * TILE;
        char* vb = kb + TILE;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int row = DMA_ROWS * (2 * wave + j) + srow;          // tile row 0..63
            const int key = min(kt * KV + row, a.seq_k - 1);
            const int kc = sch ^ ((row >> 1) & 7);                      // the source swizzles of attention_tile.h
            const int vc = sch ^ (((row >> 1) & 1) << 2);
            lds_dma16(K + (long)key * a.k_row + kc * 8, kb + (2 * wave + j) * DMA_ROWS * ROW);
            lds_dma16(V + (long)key * a.v_row + vc * 8, vb + (2 * wave + j) * DMA_ROWS * ROW);
        }
    };

    f32x16 o[2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[i][r] = 0.f;
    // row sums l[q] ride on the matrix pipe: lacc = ones^T . P^T accumulates sum_key P[key][q] into
    // every register of a 32x32 tile (the loop is VALU-bound: 4 extra MFMAs replace 32 v_add),
    // and it sums exactly the bf16-rounded P that the PV product uses
    f32x16 lacc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const bf16x8 ones = {0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80};
    float m = -INFINITY;
    const float c2 = a.scale * 1.44269504088896340736f;   // softmax scale folded into exp2

    issue(0, 0);
    wait_vmcnt<0>();   // own LDS-DMA landed, then the barrier (protocol: gfx950.h)
    __syncthreads();

    for (int kt = 0; kt < nkt; ++kt) {
        const int cur = kt & 1;
        if (kt + 1 < nkt) issue(cur ^ 1, kt + 1);
        const char* kb = smem + cur * 2 * TILE;
        const char* vb = kb + TILE;

        // ---- S^T = K Q^T : two 32-key sub-tiles ----
        f32x16 s[2];
        const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int row = t * 32 + l31;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const bf16x8 kf = (dbg & 1) ? qf[ks] :
                    *reinterpret_cast<const bf16x8*>(kb + k_frag_off(row, ks, lh));
                // the first k-step takes the constant 0 as C (inline operand: no 16-register clear)
                s[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[ks], ks == 0 ? zero16 : s[t], 0, 0, 0);
            }
        }
        // mask keys past the end (last tile only)
        if (ragged && kt == nkt - 1) {
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int key = acc_key(kt * KV + t * 32, r, lh);
                    if (key >= a.seq_k) s[t][r] = -INFINITY;
                }
        }
        // ---- online softmax (row = query = this lane, both halves) ----
        float mloc = -INFINITY;
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) mloc = fmaxf(mloc, s[t][r]);
        mloc = fmaxf(mloc, __shfl_xor(mloc, 32, 64));
        const float mnew = fmaxf(m, mloc);
        const float nmb = -(mnew * c2);
        // exact skip of the O / l rescale when no lane's running max moved (alpha == 1 for the
        // whole wave): after the first few tiles this is the common case
        if (!__all(mnew == m)) {
            const float alpha = __builtin_amdgcn_exp2f((m - mnew) * c2);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                o[0][r] *= alpha;
                o[1][r] *= alpha;
                lacc[r] *= alpha;
            }
            m = mnew;
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            // one v_fma per score (the build runs with -ffp-contract=off, so spell the fma out)
            if (!(dbg & 4)) {
                s[0][r] = __builtin_amdgcn_exp2f(__builtin_fmaf(s[0][r], c2, nmb));
                s[1][r] = __builtin_amdgcn_exp2f(__builtin_fmaf(s[1][r], c2, nmb));
            }
        }

        // ---- O^T += V^T P^T ----
#pragma unroll
        for (int t = 0; t < 2; ++t) {
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const bf16x8 pf = pack8(s[t], ks);
                if (!(dbg & 8)) lacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ones, pf, lacc, 0, 0, 0);
#pragma unroll
                for (int dt = 0; dt < 2; ++dt) {
                    bf16x8 vf = qf[0];   // the read mirrors read_vt of attention_tile.h
                    if (!(dbg & 2))
#pragma unroll
                    for (int half = 0; half < 2; ++half) {
                        const char* addr = vt_ptr(vb, t, ks, dt, half, lane, lh);
                        const s16x4 v4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)addr);
                        vf[4 * half + 0] = v4[0];
                        vf[4 * half + 1] = v4[1];
                        vf[4 * half + 2] = v4[2];
                        vf[4 * half + 3] = v4[3];
                    }
                    o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf, o[dt], 0, 0, 0);
                }
            }
        }

        wait_vmcnt<0>();   // ahead of the barrier, written out
        __syncthreads();
    }

    const float inv = 1.f / lacc[0];   // every register of lacc holds this lane's (query's) row sum
    const int q = q0 + l31;
    if (q < a.seq_q) {
        unsigned short* op = O + (long)q * a.o_row;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                bf16x4 v;
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = (short)f2x16(o[dt][4 * g + j] * inv, a.out_f16 != 0);
                *reinterpret_cast<bf16x4*>(out_ptr(op, dt, g, lh)) = v;
            }
    }
}

int attention_bf16_launch(const AttnArgs& a, const AttnPlan& p, hipStream_t st) {
    const int nqb = (int)cdiv(a.seq_q, p.queries);
    const dim3 grid((unsigned)p.grid), block(256);
    // timing ablations (wrong results) exist only in a -DSKIMI_ABLATIONS build (SKIMI_ABLATIONS=1 python -m ...build)
    switch (p.dbg) {
        default: hipLaunchKernelGGL(attn_bf16_kernel<0>, grid, block, 0, st, a, nqb); break;
#ifdef SKIMI_ABLATIONS
#define SKIMI_ABL_CASE(D) case D: hipLaunchKernelGGL(attn_bf16_kernel<D>, grid, block, 0, st, a, nqb); break;
        SKIMI_ABL_CASE(1) SKIMI_ABL_CASE(2) SKIMI_ABL_CASE(3) SKIMI_ABL_CASE(4) SKIMI_ABL_CASE(8) SKIMI_ABL_CASE(12)
        SKIMI_ABL_CASE(15)
#undef SKIMI_ABL_CASE
#endif
    }
    SKIMI_LAUNCH_CHECK();
    return SKIMI_OK;
}

}  // namespace skimi
