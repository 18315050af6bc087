// Device idioms of the MFMA kernels (gfx950): LDS-DMA pointer types, the XCD-contiguous workgroup order, s_waitcnt.
#pragma once
#include "common.h"

namespace skimi {

// operand types of __builtin_amdgcn_global_load_lds (LDS-DMA) and __builtin_amdgcn_ds_read_tr16_b64_v4i16
typedef __attribute__((address_space(3))) void lds_void;
typedef __attribute__((address_space(1))) const void gbl_void;
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

#ifdef __HIPCC__
// XCD-contiguous order of a 1-D grid.  Workgroups are dealt round-robin to the 8 XCDs, so bid and bid + 8 share an L2
// and bid and bid + 1 never do.  This maps workgroup bid of nblk to an id such that every XCD gets one contiguous run
// of ids (the first nblk % 8 XCDs one more): neighbouring ids, whose tiles share operands, meet in one L2.  Bijective
// on [0, nblk) for any nblk.
__device__ __forceinline__ int xcd_contiguous_id(int bid, int nblk) {
    const int xcd = bid & 7;
    const int q = nblk >> 3, r = nblk & 7;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
}
__device__ __forceinline__ int xcd_contiguous_id() { return xcd_contiguous_id(blockIdx.x, gridDim.x); }

// LDS-DMA (global_load_lds_dwordx4): every lane's 16 bytes at gsrc go to LDS, lane l's to ldst + 16 l (ldst is
// wave-uniform: the instruction takes ONE LDS base, 1 KiB per wave-instruction).  Counted by vmcnt, see below.
__device__ __forceinline__ void lds_dma16(const void* gsrc, void* ldst) {
    __builtin_amdgcn_global_load_lds((gbl_void*)gsrc, (lds_void*)ldst, 16, 0, 0);
}

// s_waitcnt on one counter, the other fields at their maxima (gfx9 encoding: vmcnt in bits 3:0 and 15:14, expcnt 6:4,
// lgkmcnt 11:8).  vmcnt counts this wave's outstanding global loads, LDS-DMA included, which retire in order:
// wait_vmcnt<N>() returns when at most N are in flight.  lgkmcnt counts its LDS (and scalar-memory) accesses.
//
// LDS-DMA visibility protocol of every kernel that stages tiles with global_load_lds: a wave's DMA writes are in LDS
// when ITS vmcnt says so, so every wave waits on its own DMA (wait_vmcnt<0>(), or a counted wait where later tiles
// stay in flight) and only then enters the workgroup barrier; after the barrier all waves' shares of the tile are
// there.  The wait is written out, not left to how hipcc lowers __syncthreads(): gfx950 barriers do not wait for
// memory counters by themselves.  tests/test_abi.py looks for `s_waitcnt vmcnt(0)` ahead of every s_barrier of
// attn_q64_kernel in the emitted ISA.
constexpr int vmcnt_imm(int n) { return 0x0F70 | (n & 15) | ((n >> 4) << 14); }
static_assert(vmcnt_imm(0) == 0x0F70 && vmcnt_imm(5) == 0x0F75 && vmcnt_imm(24) == 0x4F78, "s_waitcnt vmcnt encoding");
template <int N>
__device__ __forceinline__ void wait_vmcnt() {
    static_assert(N >= 0 && N < 64, "vmcnt is a 6-bit counter");
    __builtin_amdgcn_s_waitcnt(vmcnt_imm(N));
}
__device__ __forceinline__ void wait_lgkmcnt0() { __builtin_amdgcn_s_waitcnt(0xC07F); }
// raw s_barrier (no memory-counter waits added by the compiler) that the scheduler moves nothing across
__device__ __forceinline__ void fenced_barrier() {
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
}
#endif

}  // namespace skimi
