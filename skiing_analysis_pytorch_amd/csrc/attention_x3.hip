// fp32-accurate flash attention for head_dim 64 on the bf16 matrix pipe (the attention of SKIMI_PREC_BF16X3, the
// parity mode): every operand is x = hi + lo (two bf16), every product three MFMAs (lo*hi + hi*lo + hi*hi), as
// the bf16x3 GEMMs do.  The exact-fp32 kernel (attention_f32.hip, v_mfma_f32_32x32x2_f32) runs at 65 TFLOP/s and
// made attention three quarters of a parity-mode step (228 of 290 ms per 8-view step); this one is bound by
// 50 MFMAs per 64-key tile and 32 queries.
//
// Structure = attention_bf16.hip's 32-query kernel: 4 waves x 32 queries per workgroup, swapped products
// (S^T = K Q^T, O^T += V^T P^T, a softmax row per lane pair), K / V tiles of 64 keys double-buffered in LDS by
// LDS-DMA -- here FOUR tiles per stage (K hi, K lo, V hi, V lo: 32 KiB, 64 KiB for the two stages, two
// workgroups per CU), streamed from the hi / lo bf16 planes that split_planes_kernel makes of the fp32 qkv
// buffer once per call (the split is then not repeated by every query block).  Q is read as fp32, multiplied
// by scale x log2(e) and split in registers, so the scores arrive in log2 units and the softmax is
// v_sub + v_exp2 per score in fp32; P is split like every other operand (p_hi = bf16(p), p_lo = bf16(p - p_hi));
// row sums are fp32 VALU adds of the unsplit p.  Output fp32.
#include <stdlib.h>

#include "attention_tile.h"
#include "common.h"
#include "gemm_epilogue.h"
#include "kernels.h"

namespace skimi {

struct AttnX3Args {
    const float* q;                       // fp32, AttnArgs strides (elements)
    const unsigned short *khi, *klo, *vhi, *vlo;   // bf16 planes, the same element strides
    float* out;
    unsigned short* out_rec;              // or null: the result as bf16x3 records [token][C / 32][hi 32 | lo 32] instead of fp32
    long rec_row, rec_batch;              // ushorts per token row / per batch element
    long q_row, k_row, v_row, o_row, q_batch, k_batch, v_batch, o_batch, q_head, k_head, v_head, o_head;
    int batch, heads, seq_q, seq_k;
    float scale;
};

using namespace att;   // the K / V tile layout shared with attention_bf16.hip and attention_q64.hip

__global__ __launch_bounds__(256, 2) void attn_x3_kernel(const AttnX3Args a, int nqb) {
    __shared__ __attribute__((aligned(16))) char smem[8 * TILE];   // [buf][K hi | K lo | V hi | V lo]

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, lh = lane >> 5;
    const int id = xcd_contiguous_id();   // one XCD's L2 holds a head's K/V planes
    const int qb = id % nqb;
    const int bh = id / nqb;
    const int head = bh % a.heads, b = bh / a.heads;
    const int q0 = qb * 128 + wave * 32;

    const long koff = (long)b * a.k_batch + (long)head * a.k_head, voff = (long)b * a.v_batch + (long)head * a.v_head;
    const unsigned short *Kh = a.khi + koff, *Kl = a.klo + koff, *Vh = a.vhi + voff, *Vl = a.vlo + voff;

    // Q fragments (B operand): lane (q, h) holds Q[q][16 s + 8 h + j] * scale * log2(e), split hi + lo
    bf16x8 qh[4], ql[4];
    {
        const int q = min(q0 + l31, a.seq_q - 1);
        const float* qp = a.q + (long)b * a.q_batch + (long)head * a.q_head + (long)q * a.q_row + 8 * lh;
        const float c2 = a.scale * 1.44269504088896340736f;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const float4 v0 = *reinterpret_cast<const float4*>(qp + 16 * s);
            const float4 v1 = *reinterpret_cast<const float4*>(qp + 16 * s + 4);
            const float f[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float x = f[j] * c2;
                const unsigned short hb = f2bf(x);
                qh[s][j] = (short)hb;
                ql[s][j] = (short)f2bf(x - bf2f(hb));
            }
        }
    }

    const int nkt = (a.seq_k + KV - 1) / KV;
    const bool ragged = (a.seq_k & (KV - 1)) != 0;
    const int srow = lane >> 3, sch = lane & 7;
    auto issue = [&](int buf, int kt) {
        char* base = smem + buf * 4 * TILE;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int row = DMA_ROWS * (2 * wave + j) + srow;
            const int key = min(kt * KV + row, a.seq_k - 1);
            const int kc = sch ^ ((row >> 1) & 7);                      // the source swizzles of attention_tile.h
            const int vc = sch ^ (((row >> 1) & 1) << 2);
            const int dst = (2 * wave + j) * DMA_ROWS * ROW;
            lds_dma16(Kh + (long)key * a.k_row + kc * 8, base + dst);
            lds_dma16(Kl + (long)key * a.k_row + kc * 8, base + TILE + dst);
            lds_dma16(Vh + (long)key * a.v_row + vc * 8, base + 2 * TILE + dst);
            lds_dma16(Vl + (long)key * a.v_row + vc * 8, base + 3 * TILE + dst);
        }
    };

    f32x16 o[2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[i][r] = 0.f;
    float lsum = 0.f;          // this lane's partial row sum (its 32 of every 64 keys)
    float m = -INFINITY;
    const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};

    issue(0, 0);
    wait_vmcnt<0>();   // own LDS-DMA landed, then the barrier (protocol: gfx950.h)
    __syncthreads();

    for (int kt = 0; kt < nkt; ++kt) {
        const int cur = kt & 1;
        if (kt + 1 < nkt) issue(cur ^ 1, kt + 1);
        const char* kbh = smem + cur * 4 * TILE;
        const char* kbl = kbh + TILE;
        const char* vbh = kbh + 2 * TILE;
        const char* vbl = kbh + 3 * TILE;

        // ---- S^T = K Q^T, three terms, small ones first ----
        f32x16 s[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int row = t * 32 + l31;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const int off = k_frag_off(row, ks, lh);
                const bf16x8 kfh = *reinterpret_cast<const bf16x8*>(kbh + off);
                const bf16x8 kfl = *reinterpret_cast<const bf16x8*>(kbl + off);
                s[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kfl, qh[ks], ks == 0 ? zero16 : s[t], 0, 0, 0);
                s[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kfh, ql[ks], s[t], 0, 0, 0);
                s[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kfh, qh[ks], s[t], 0, 0, 0);
            }
        }
        if (ragged && kt == nkt - 1) {
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int key = acc_key(kt * KV + t * 32, r, lh);
                    if (key >= a.seq_k) s[t][r] = -INFINITY;
                }
        }
        // ---- online softmax in fp32 (scores are in log2 units) ----
        float mloc = -INFINITY;
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) mloc = fmaxf(mloc, s[t][r]);
        mloc = fmaxf(mloc, __shfl_xor(mloc, 32, 64));
        const float mnew = fmaxf(m, mloc);
        if (!__all(mnew == m)) {   // exact skip when no row's maximum moved
            const float alpha = __builtin_amdgcn_exp2f(m - mnew);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                o[0][r] *= alpha;
                o[1][r] *= alpha;
            }
            lsum *= alpha;
            m = mnew;
        }
        float l0 = 0.f, l1 = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            s[0][r] = __builtin_amdgcn_exp2f(s[0][r] - mnew);
            s[1][r] = __builtin_amdgcn_exp2f(s[1][r] - mnew);
            l0 += s[0][r];
            l1 += s[1][r];
        }
        lsum += l0 + l1;

        // ---- O^T += V^T P^T, P split like every other operand ----
#pragma unroll
        for (int t = 0; t < 2; ++t) {
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                bf16x8 ph, pl;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float p = s[t][8 * ks + j];
                    const unsigned short hb = f2bf(p);
                    ph[j] = (short)hb;
                    pl[j] = (short)f2bf(p - bf2f(hb));
                }
#pragma unroll
                for (int dt = 0; dt < 2; ++dt) {
                    const bf16x8 vfh = read_vt(vbh, t, ks, dt, lane, lh);
                    const bf16x8 vfl = read_vt(vbl, t, ks, dt, lane, lh);
                    o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vfl, ph, o[dt], 0, 0, 0);
                    o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vfh, pl, o[dt], 0, 0, 0);
                    o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vfh, ph, o[dt], 0, 0, 0);
                }
            }
        }
        wait_vmcnt<0>();   // ahead of the barrier, written out
        __syncthreads();
    }

    const float tot = lsum + __shfl_xor(lsum, 32, 64);
    const float inv = 1.f / tot;
    const int q = q0 + l31;
    if (a.out_rec != nullptr) {
        // records for the proj GEMM (no fp32 copy, no split pass).  A lane pair holds a row's 64 values as 4-element pieces
        // alternating between its two halves; one v_permlane32_swap per value pair gives every lane 8 consecutive elements
        // (lh = 0: the even 8-element groups, lh = 1: the odd ones), i.e. one 16-byte hi and one 16-byte lo store each.
        unsigned short* rp = a.out_rec + (long)b * a.rec_batch + (long)q * a.rec_row + (long)head * 128;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int pr = 0; pr < 2; ++pr) {
                float w[8];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(o[dt][8 * pr + j] * inv),
                                                                    __float_as_uint(o[dt][8 * pr + 4 + j] * inv), false, false);
                    w[j] = __uint_as_float(r[0]);
                    w[4 + j] = __uint_as_float(r[1]);
                }
                bf16x8 h8, l8;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const unsigned short hb = f2bf(w[j]);
                    h8[j] = (short)hb;
                    l8[j] = (short)f2bf(w[j] - bf2f(hb));
                }
                if (q < a.seq_q) {
                    unsigned short* sp = rp + dt * 64 + 8 * (2 * pr + lh);
                    *reinterpret_cast<bf16x8*>(sp) = h8;
                    *reinterpret_cast<bf16x8*>(sp + 32) = l8;
                }
            }
        return;
    }
    if (q < a.seq_q) {
        float* op = a.out + (long)b * a.o_batch + (long)head * a.o_head + (long)q * a.o_row;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int g = 0; g < 4; ++g)
                *reinterpret_cast<float4*>(out_ptr(op, dt, g, lh)) =
                    make_float4(o[dt][4 * g] * inv, o[dt][4 * g + 1] * inv, o[dt][4 * g + 2] * inv, o[dt][4 * g + 3] * inv);
    }
}

size_t attention_x3_scratch_bytes(long tokens, long row_elems) { return (size_t)tokens * row_elems * 4 + 512; }

// a: fp32 AttnArgs of ONE packed buffer (rows [q | k | v] of a.q_row floats starting at a.q); p: plan_attention's plane
// layout -- only k and v are read as planes (q is split in registers), so the planes hold just columns c0 .. c0 + pw.
// scratch: >= attention_x3_scratch_bytes: the hi / lo planes.
// p.out_form ATTN_OUT_RECORDS: a.out (128-byte aligned, a plain [tokens, heads * 64] result) receives bf16x3 records
// [tokens][heads * 64 / 32][hi 32 | lo 32] (+ 256 zero bytes behind them) instead of fp32 rows -- the operand form of the
// proj GEMM on the LDS-DMA bf16x3 kernel
int attention_x3_launch(const AttnArgs& a, const AttnPlan& p, void* scratch, hipStream_t st) {
    const long tokens = (long)a.batch * a.seq_q, row_elems = a.q_row;
    const float* base = (const float*)a.q;
    unsigned short* hi = (unsigned short*)(((uintptr_t)scratch + 255) & ~(uintptr_t)255);
    unsigned short* lo = hi + tokens * p.pw;
    int rc = split_planes_launch(base + p.c0, row_elems, tokens, (int)p.pw, hi, lo, st);
    if (rc) return rc;
    AttnX3Args x;
    x.q = base; x.khi = hi + p.koff; x.klo = lo + p.koff; x.vhi = hi + p.voff; x.vlo = lo + p.voff; x.out = (float*)a.out;
    x.q_row = a.q_row; x.k_row = x.v_row = p.pw; x.o_row = a.o_row;
    x.q_batch = a.q_batch; x.o_batch = a.o_batch;
    x.k_batch = a.k_batch / row_elems * p.pw;
    x.v_batch = a.v_batch / row_elems * p.pw;
    x.q_head = a.q_head; x.k_head = a.k_head; x.v_head = a.v_head; x.o_head = a.o_head;
    x.batch = a.batch; x.heads = a.heads; x.seq_q = a.seq_q; x.seq_k = a.seq_k; x.scale = a.scale;
    x.out_rec = nullptr; x.rec_row = 0; x.rec_batch = 0;
    if (p.out_form == ATTN_OUT_RECORDS) {
        x.out_rec = (unsigned short*)a.out;
        x.rec_row = a.o_row * 2;               // 4 bytes per element: [hi 32 | lo 32] per 32-column slice
        x.rec_batch = (long)a.seq_q * x.rec_row;
        if (hipMemsetAsync((char*)a.out + (size_t)tokens * a.o_row * 4, 0, 256, st) != hipSuccess) {   // the zero page behind the records
            set_error("hipMemsetAsync(attention records zero page) failed");
            return SKIMI_ERR_HIP;
        }
    }
    hipLaunchKernelGGL(attn_x3_kernel, dim3((unsigned)p.grid), dim3(256), 0, st, x, (int)cdiv(a.seq_q, p.queries));
    SKIMI_LAUNCH_CHECK();
    return SKIMI_OK;
}

}  // namespace skimi
