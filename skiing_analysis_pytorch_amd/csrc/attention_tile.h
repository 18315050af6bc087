// The K / V tile of the three head_dim-64 flash-attention kernels (attention_bf16.hip, attention_q64.hip,
// attention_x3.hip): everything one of them has to spell like the other two in order to be correct.
//
// Products are swapped (S^T = K Q^T, O^T += V^T P^T on v_mfma_f32_32x32x16_bf16), so a softmax row is one lane pair
// (lane & 31 = query, lh = lane >> 5).  A tile is 64 keys x 64 bf16, row-major [key][d], 128 B per row, staged by
// LDS-DMA (gfx950.h has the visibility protocol: own wait_vmcnt<0>(), then the workgroup barrier).  One DMA
// wave-instruction lands 8 rows linearly (lane l: row l >> 3, 16-B chunk l & 7), so both bank swizzles are applied to
// the per-lane SOURCE chunk and undone by the readers' addresses:
//   K rows: chunk ^= (row >> 1) & 7          conflict-free ds_read_b128 of 32 rows at one chunk
//   V rows: chunk ^= ((row >> 1) & 1) << 2   conflict-free ds_read_b64_tr_b16 of 4-row blocks
// (the stagers spell the two XORs out: kc / vc of their `issue` lambdas; k_frag_off and vt_ptr are the read sides).
// Rows past the end of the sequence are clamped to the last key by the stager and masked to -inf by key index.
#pragma once
#include "gfx950.h"

namespace skimi {
namespace att {

constexpr int KV = 64;           // keys per tile
constexpr int ROW = 128;         // bytes per tile row (64 bf16 of one key)
constexpr int TILE = KV * ROW;   // bytes of one K (or V) tile
constexpr int DMA_ROWS = 8;      // tile rows per LDS-DMA wave-instruction

#ifdef __HIPCC__
// The helpers are shaped after the sums they replace (base + ... where a kernel added to a base): hipcc keeps the
// association, and the kernels' assembly was to stay as it was (profiles/shared_mfma_helpers.md).
// K, read side: byte offset in the tile of the A fragment of key `row` for k-step ks (d = 16 ks + 8 lh .. + 7)
__device__ __forceinline__ constexpr int k_frag_off(int row, int ks, int lh) {
    return row * ROW + (((2 * ks + lh) ^ ((row >> 1) & 7)) << 4);
}

// V, read side: address of one ds_read_b64_tr_b16 (4-row x 4-column transpose blocks) of the V^T fragment for keys
// key0 = 32 t + 16 ks + 8 half .. + 7 and d tile dt: row key0 + 4 lh + ((lane & 15) >> 2), 4 columns from dcol
__device__ __forceinline__ const char* vt_ptr(const char* vb, int t, int ks, int dt, int half, int lane, int lh) {
    const int q4 = (lane & 15) >> 2, p4 = lane & 3;
    const int dcol = dt * 32 + 16 * ((lane >> 4) & 1) + 4 * p4;
    const int row = t * 32 + 16 * ks + 8 * half + 4 * lh + q4;
    const int chunk = (dcol >> 3) ^ (((row >> 1) & 1) << 2);
    return vb + row * ROW + (chunk << 4) + ((dcol & 7) << 1);
}
// the whole V^T fragment (A operand of O^T += V^T P^T)
__device__ __forceinline__ bf16x8 read_vt(const char* vb, int t, int ks, int dt, int lane, int lh) {
    bf16x8 vf;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const s16x4 v4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)vt_ptr(vb, t, ks, dt, half, lane, lh));
        vf[4 * half + 0] = v4[0];
        vf[4 * half + 1] = v4[1];
        vf[4 * half + 2] = v4[2];
        vf[4 * half + 3] = v4[3];
    }
    return vf;
}

// key order: the key in register r of the S^T accumulator of the 32-key block at key0 (= P's k order in the PV product)
__device__ __forceinline__ constexpr int acc_key(int key0, int r, int lh) { return key0 + (r & 3) + 8 * (r >> 2) + 4 * lh; }
// where a lane's output goes: registers 4 g .. 4 g + 3 of O^T accumulator dt are d columns dt * 32 + 8 g + 4 lh .. + 3
template <typename T>
__device__ __forceinline__ T* out_ptr(T* row, int dt, int g, int lh) { return row + dt * 32 + 8 * g + 4 * lh; }

// max / sum of a value over the lane pair (l, l ^ 32): one v_permlane32_swap, no LDS
__device__ __forceinline__ float xhalf_max(float x) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return __builtin_fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
__device__ __forceinline__ float xhalf_sum(float x) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
#endif

}  // namespace att
}  // namespace skimi
