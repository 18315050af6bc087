// Measured peaks of THIS MI355X (BASELINE.md §3 asks for them beside the datasheet 2.5 PFLOP/s / 8 TB/s that
// bench.py prices against): a register-only v_mfma_f32_32x32x16_bf16 loop (every SIMD busy, no memory) on zero
// and on random operands (the part is power-limited: MI355X_MICROARCH.md), and streaming reads / copies of a 4 GiB
// buffer at 16 B per lane.  Since round 4 every MFMA variant is priced by its own MFMA count (the round-3 file priced
// the 16x16x32 loop, 16 MFMAs of 16384 FLOP per iteration, as 4 of 32768: half its FLOPs), the two shapes are also run
// fed from LDS the way gemm256w4_kernel feeds them, and every variant reports its wall time and its in-kernel clock
// (s_memtime / s_memrealtime stamped once around the loop, median over workgroups).  Build + run:
//   hipcc --offload-arch=gfx950 -O3 tools/peaks.hip -o tools/_peaks && tools/_peaks > profiles/r04_peaks.json
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <vector>

typedef __attribute__((ext_vector_type(8))) short bf16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) float f32x4;

__global__ __launch_bounds__(256) void mfma_loop(const bf16x8* in, float* out, int iters) {
    const bf16x8 a = in[threadIdx.x], b = in[256 + threadIdx.x];
    f32x16 acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc[i], 0, 0, 0);
    }
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) s += acc[i][0] + acc[i][7];
    if (s == 123.456f) out[0] = s;   // keep the loop
}

// the same loop on the other shape / format: SHAPE 0 = 32x32x16 (4 accumulators, 4 MFMAs = 131072 FLOP per wave and
// iteration), 1 = 16x16x32 (16 accumulators of 4 registers: the same 64 accumulator registers, 16 MFMAs = 262144 FLOP
// per wave and iteration: twice the FLOPs of SHAPE 0); F16: fp16 operands instead of bf16
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
static double flop_per_wave_iter(int shape) { return shape == 0 ? 4 * 32768.0 : 16 * 16384.0; }

// clock stamps of one workgroup (thread 0): s_memtime ticks (shader clock) and s_memrealtime ticks (100 MHz) across its loop
__device__ __forceinline__ void stamp(unsigned long long& t, unsigned long long& r) {
    __builtin_amdgcn_sched_barrier(0);
    t = __builtin_amdgcn_s_memtime();
    r = __builtin_amdgcn_s_memrealtime();
    __builtin_amdgcn_s_waitcnt(0xC07F);
    __builtin_amdgcn_sched_barrier(0);
}

template <bool F16>
__device__ __forceinline__ void loop32(const bf16x8 a, const bf16x8 b, float* out, int iters) {
    const f16x8 ah = __builtin_bit_cast(f16x8, a), bh = __builtin_bit_cast(f16x8, b);
    f32x16 acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            // inline asm with the accumulators pinned in VGPRs: hipcc's allocator otherwise shuttles half of the 16x16
            // accumulators through v_accvgpr_mov every iteration
            if constexpr (F16) asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, %0" : "+a"(acc[i]) : "v"(ah), "v"(bh));
            else asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+a"(acc[i]) : "v"(a), "v"(b));
        }
    }
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) s += acc[i][0] + acc[i][7];
    if (s == 123.456f) out[0] = s;
}
template <bool F16>
__device__ __forceinline__ void loop16(const bf16x8 a, const bf16x8 b, float* out, int iters) {
    const f16x8 ah = __builtin_bit_cast(f16x8, a), bh = __builtin_bit_cast(f16x8, b);
    f32x4 acc[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            if constexpr (F16) asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+a"(acc[i]) : "v"(ah), "v"(bh));
            else asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+a"(acc[i]) : "v"(a), "v"(b));
        }
    }
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) s += acc[i][0] + acc[i][3];
    if (s == 123.456f) out[0] = s;
}
template <int SHAPE, bool F16>
__global__ __launch_bounds__(256) void mfma_loop2(const bf16x8* in, float* out, int iters, unsigned long long* st) {
    const bf16x8 a = in[threadIdx.x], b = in[256 + threadIdx.x];
    unsigned long long t0, r0, t1, r1;
    stamp(t0, r0);
    if constexpr (SHAPE == 0) loop32<F16>(a, b, out, iters);
    else loop16<F16>(a, b, out, iters);
    stamp(t1, r1);
    if (threadIdx.x == 0) { st[2 * blockIdx.x] = t1 - t0; st[2 * blockIdx.x + 1] = r1 - r0; }
}

// LDS-fed loop, one workgroup of 4 waves per CU (one wave per SIMD), like gemm256w4_kernel: one 64-deep K-tile of a
// 256x256 output tile sits in LDS as two [256][128 B] row images (16-B chunk ^= (row >> 1) & 7), every wave owns a
// 128x128 quadrant (256 accumulator registers) and re-reads all its A / B fragments with ds_read_b128 every K-tile.
//   SHAPE 0: 4 k-steps of 16, each 4 + 4 fragments and 16 v_mfma_f32_32x32x16  (rows l & 31, chunk 2 s + (l >> 5))
//   SHAPE 1: 2 k-steps of 32, each 8 + 8 fragments and 64 v_mfma_f32_16x16x32  (rows l & 15, chunk 4 s + (l >> 4))
// Both: 128 * 128 * 64 * 2 FLOP and 32 fragment reads per wave and K-tile.  Inline-asm MFMAs with the accumulators
// pinned in AGPRs, as in the register loops (with the builtin, hipcc rotates 60 accumulator registers through
// v_accvgpr_mov every iteration of the 16x16x32 loop and none of the 32x32x16 loop).
template <int SHAPE, bool F16>
__global__ __launch_bounds__(256, 1) void mfma_lds_loop(const bf16x8* in, float* out, int iters, unsigned long long* st) {
    __shared__ bf16x8 lds[2 * 256 * 8];   // 64 KiB: A rows, then B rows
    for (int i = threadIdx.x; i < 2 * 256 * 8; i += 256) {
        const int row = (i >> 3) & 255;
        lds[(i & ~7) + ((i & 7) ^ ((row >> 1) & 7))] = in[i];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const char* pa = reinterpret_cast<const char*>(lds) + (128 * (wave >> 1)) * 128;
    const char* pb = reinterpret_cast<const char*>(lds) + (256 + 128 * (wave & 1)) * 128;
    unsigned long long t0, r0, t1, r1;
    float s = 0.f;
    stamp(t0, r0);
    if constexpr (SHAPE == 0) {
        f32x16 acc[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
        const int l31 = lane & 31, lh = lane >> 5;
        for (int it = 0; it < iters; ++it) {
            asm volatile("" ::: "memory");   // the tile is re-read every iteration
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                bf16x8 fa[4], fb[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int row = 32 * i + l31;
                    fa[i] = *reinterpret_cast<const bf16x8*>(pa + row * 128 + (((2 * k + lh) ^ ((row >> 1) & 7)) << 4));
                    fb[i] = *reinterpret_cast<const bf16x8*>(pb + row * 128 + (((2 * k + lh) ^ ((row >> 1) & 7)) << 4));
                }
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        if constexpr (F16) asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, %0" : "+a"(acc[i][j]) : "v"(fa[i]), "v"(fb[j]));
                        else asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+a"(acc[i][j]) : "v"(fa[i]), "v"(fb[j]));
                    }
            }
        }
        stamp(t1, r1);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) s += acc[i][j][0] + acc[i][j][15];
    } else {
        f32x4 acc[8][8];
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        const int l15 = lane & 15, lq = lane >> 4;
        for (int it = 0; it < iters; ++it) {
            asm volatile("" ::: "memory");
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                bf16x8 fa[8], fb[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const int row = 16 * i + l15;
                    fa[i] = *reinterpret_cast<const bf16x8*>(pa + row * 128 + (((4 * k + lq) ^ ((row >> 1) & 7)) << 4));
                    fb[i] = *reinterpret_cast<const bf16x8*>(pb + row * 128 + (((4 * k + lq) ^ ((row >> 1) & 7)) << 4));
                }
#pragma unroll
                for (int i = 0; i < 8; ++i)
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        if constexpr (F16) asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+a"(acc[i][j]) : "v"(fa[i]), "v"(fb[j]));
                        else asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+a"(acc[i][j]) : "v"(fa[i]), "v"(fb[j]));
                    }
            }
        }
        stamp(t1, r1);
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int j = 0; j < 8; ++j) s += acc[i][j][0] + acc[i][j][3];
    }
    if (threadIdx.x == 0) { st[2 * blockIdx.x] = t1 - t0; st[2 * blockIdx.x + 1] = r1 - r0; }
    if (s == 123.456f) out[0] = s;
}

__global__ __launch_bounds__(256) void stream_read(const f32x4* x, long n, float* out) {
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) s += __builtin_nontemporal_load(x + i);
    if (s[0] + s[1] + s[2] + s[3] == 123.456f) out[0] = s[0];
}
__global__ __launch_bounds__(256) void stream_copy(const f32x4* x, f32x4* y, long n) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) __builtin_nontemporal_store(__builtin_nontemporal_load(x + i), y + i);
}

template <typename F>
static double time_ms(F f, int reps) {
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    f();
    hipDeviceSynchronize();
    hipEventRecord(e0);
    for (int i = 0; i < reps; ++i) f();
    hipEventRecord(e1);
    hipEventSynchronize(e1);
    float ms;
    hipEventElapsedTime(&ms, e0, e1);
    return ms / reps;
}

int main() {
    std::vector<unsigned short> h(512 * 8);
    bf16x8* din;
    float* dout;
    hipMalloc(&din, 512 * 16);
    hipMalloc(&dout, 64);
    const int iters = 20000, blocks = 256 * 8;   // 8 workgroups of 4 waves per CU: 8 waves per SIMD
    double tf[2];
    for (int pass = 0; pass < 2; ++pass) {
        srand(1);
        for (auto& v : h) v = pass == 0 ? 0 : (unsigned short)(0x3C00 + (rand() & 0x3FF) + ((rand() & 1) << 15));   // |x| in [0.0078, 0.0156), random sign
        hipMemcpy(din, h.data(), 512 * 16, hipMemcpyHostToDevice);
        const double ms = time_ms([&] { mfma_loop<<<blocks, 256>>>(din, dout, iters); }, 3);
        tf[pass] = (double)blocks * 4 * iters * 4 * 32768.0 / (ms * 1e-3) / 1e12;
    }
    // MFMA shape x operand format on random operands (MI355X_MICROARCH.md "DVFS give-back" (7): the clock the chip holds
    // under load depends on the MFMA shape): register-only loops at 1 and 8 waves per SIMD, the LDS-fed loop at 1 wave
    // per SIMD.  Each variant: 1 s of back-to-back launches (clock settled), then 0.5 s timed; the four variants of a
    // group interleaved twice.  Clock = median over workgroups of the last launch's s_memtime / s_memrealtime ticks.
    {
        const int nlds = 2 * 256 * 8;
        std::vector<unsigned short> hr(nlds * 8);
        srand(1);
        // values with random mantissas that are ordinary numbers in BOTH formats: bf16 0x3C00.. = 0.0078.., fp16 0x3C00.. = 1.0..
        for (auto& v : hr) v = (unsigned short)(0x3C00 + (rand() & 0x3FF) + ((rand() & 1) << 15));
        bf16x8* dr;
        hipMalloc(&dr, nlds * 16);
        hipMemcpy(dr, hr.data(), nlds * 16, hipMemcpyHostToDevice);
        unsigned long long* dst;
        hipMalloc(&dst, 2 * 2048 * 8);
        std::vector<unsigned long long> hst(2 * 2048);
        struct Res { double ms = 0, tf = 0, ghz = 0; };
        // runs f (nb workgroups) for ~1 s, then times it for ~0.5 s; returns wall per launch and the in-kernel clock
        auto measure = [&](auto f, int nb, double flop, Res& out) {
            const double ms1 = time_ms(f, 1);
            const int warm = (int)(1000.0 / ms1) + 1, reps = (int)(500.0 / ms1) + 1;
            for (int i = 0; i < warm; ++i) f();
            const double ms = time_ms(f, reps);
            hipMemcpy(hst.data(), dst, 2 * nb * 8, hipMemcpyDeviceToHost);
            std::vector<double> c(nb);
            for (int b = 0; b < nb; ++b) c[b] = (double)hst[2 * b] / (double)hst[2 * b + 1] * 0.1;   // GHz
            std::sort(c.begin(), c.end());
            out.ms += ms / 2;
            out.tf += flop / (ms * 1e-3) / 1e12 / 2;
            out.ghz += c[nb / 2] / 2;
        };
        const char* names[4] = {"bf16_32x32x16", "bf16_16x16x32", "f16_32x32x16", "f16_16x16x32"};
        auto print_group = [&](const char* key, Res (&r)[4], const char* tail) {
            printf("  \"%s\": {", key);
            for (int v = 0; v < 4; ++v)
                printf("\"%s\": {\"TFLOPs\": %.0f, \"wall_ms\": %.3f, \"clock_GHz\": %.3f}, ", names[v], r[v].tf, r[v].ms, r[v].ghz);
            printf("\"ratio_16x16x32_over_32x32x16\": {\"bf16\": %.3f, \"f16\": %.3f}}%s\n", r[1].tf / r[0].tf, r[3].tf / r[2].tf, tail);
        };
        printf("{\n \"mfma_shape_format_random_operands\": {\n");
        for (int wps = 1; wps <= 8; wps *= 8) {
            const int nb = 256 * wps;
            Res r[4];
            for (int rep = 0; rep < 2; ++rep) {
                measure([&] { mfma_loop2<0, false><<<nb, 256>>>(dr, dout, iters, dst); }, nb, (double)nb * 4 * iters * flop_per_wave_iter(0), r[0]);
                measure([&] { mfma_loop2<1, false><<<nb, 256>>>(dr, dout, iters, dst); }, nb, (double)nb * 4 * iters * flop_per_wave_iter(1), r[1]);
                measure([&] { mfma_loop2<0, true><<<nb, 256>>>(dr, dout, iters, dst); }, nb, (double)nb * 4 * iters * flop_per_wave_iter(0), r[2]);
                measure([&] { mfma_loop2<1, true><<<nb, 256>>>(dr, dout, iters, dst); }, nb, (double)nb * 4 * iters * flop_per_wave_iter(1), r[3]);
            }
            char key[64];
            snprintf(key, sizeof key, "register_loop_%d_waves_per_simd", wps);
            print_group(key, r, ",");
        }
        {
            const int nb = 256, lit = 4000;
            const double fl = (double)nb * 4 * lit * (128.0 * 128 * 64 * 2);
            Res r[4];
            for (int rep = 0; rep < 2; ++rep) {
                measure([&] { mfma_lds_loop<0, false><<<nb, 256>>>(dr, dout, lit, dst); }, nb, fl, r[0]);
                measure([&] { mfma_lds_loop<1, false><<<nb, 256>>>(dr, dout, lit, dst); }, nb, fl, r[1]);
                measure([&] { mfma_lds_loop<0, true><<<nb, 256>>>(dr, dout, lit, dst); }, nb, fl, r[2]);
                measure([&] { mfma_lds_loop<1, true><<<nb, 256>>>(dr, dout, lit, dst); }, nb, fl, r[3]);
            }
            print_group("lds_fed_loop_1_wave_per_simd_128x128_per_wave", r, "");
        }
        printf(" },\n");
    }
    const long n = (4l << 30) / 16;
    f32x4 *x, *y;
    hipMalloc(&x, n * 16);
    hipMalloc(&y, n * 16);
    hipMemset(x, 1, n * 16);
    const double rd = time_ms([&] { stream_read<<<256 * 16, 256>>>(x, n, dout); }, 5);
    const double cp = time_ms([&] { stream_copy<<<256 * 16, 256>>>(x, y, n); }, 5);
    printf(" \"device\": \"MI355X (gfx950)\",\n \"mfma_bf16_32x32x16_register_loop_TFLOPs\": {\"zero_operands\": %.0f, \"random_operands\": %.0f, \"datasheet_dense\": 2500},\n"
           " \"hbm_stream_4GiB_GBps\": {\"read\": %.0f, \"copy_read_plus_write\": %.0f, \"datasheet\": 8000},\n"
           " \"note\": \"bench.py prices roofline.frac against the datasheet peaks (MI355X_MICROARCH.md); these are what this box delivers on a loop with no memory traffic / no compute\"\n}\n",
           tf[0], tf[1], n * 16.0 / (rd * 1e-3) / 1e9, 2.0 * n * 16.0 / (cp * 1e-3) / 1e9);
    return 0;
}
