// Fused MFMA contraction for gfx950:  out = epilogue( gather(A) . W^T )
//
// One kernel template serves every Linear / Conv1d / Conv2d / ConvTranspose2d(k==s) on
// the hot path (reference: vggt/vggt/layers/{attention,mlp,patch_embed}.py,
// vggt/vggt/heads/dpt_head.py, VideoPose3D/common/model.py:126-138):
//   * A is channels-last; "plain" rows or an implicit-im2col gather of a KHxKW window
//     (tap-major K), so a 3x3 conv is 9 shifted GEMM-accumulates with no im2col buffer;
//   * W is [N, K] (nn.Linear layout; conv weights are repacked [Cout, ky, kx, Cin] once);
//   * 128x128 (or 64x64) output tile per 256-thread workgroup, 4 waves as 2x2, each wave
//     a 2x2 (1x1) grid of v_mfma_f32_32x32x16_bf16 tiles, fp32 accumulate;
//   * operands staged global -> VGPR -> LDS (issue early, write after the MFMA phase),
//     two LDS buffers, one barrier per K-tile; LDS rows XOR-swizzled per 16-B chunk so the
//     ds_read_b128 fragment reads are bank-conflict free;
//   * PREC_BF16X3 keeps fp32 operands in HBM and splits them hi+lo while staging:
//     acc += Ahi*Whi + Ahi*Wlo + Alo*Whi  (three MFMAs per k-step, ~fp32 operand accuracy);
//   * split-K (grid.y) stores fp32 partials into one slab plane per split and a second small
//     kernel adds the planes in split order (run-to-run identical) and applies the epilogue —
//     used when M is too small to fill 256 CUs;
//   * blockIdx -> tile map is XCD-aware: each XCD walks a contiguous run of tiles that share
//     an A row panel, so the panel and W stay in that XCD's L2.
#include "common.h"
#include "env.h"
#include "gemm_epilogue.h"
#include "gfx950.h"
#include <algorithm>
#include <stdlib.h>

namespace skimi {

// ---- staging helpers ------------------------------------------------------------------
template <typename T> struct Stage;
template <> struct Stage<float> { float4 a, b; };
template <> struct Stage<unsigned short> { bf16x8 v; };

// Loads are UNCONDITIONAL (the caller clamps the address into the buffer): a predicated load
// compiles to a branch plus a vmcnt(0) at its join, which serialises the whole staging burst.
// Out-of-range chunks are zeroed in registers (v_cndmask) when they are parked in LDS.
__device__ __forceinline__ void stage_load(Stage<float>& s, const float* p) {
    s.a = *reinterpret_cast<const float4*>(p);
    s.b = *reinterpret_cast<const float4*>(p + 4);
}
__device__ __forceinline__ void stage_load(Stage<unsigned short>& s, const unsigned short* p) {
    s.v = *reinterpret_cast<const bf16x8*>(p);
}
__device__ __forceinline__ void stage_mask(Stage<float>& s, bool ok) {
    s.a.x = ok ? s.a.x : 0.f; s.a.y = ok ? s.a.y : 0.f; s.a.z = ok ? s.a.z : 0.f; s.a.w = ok ? s.a.w : 0.f;
    s.b.x = ok ? s.b.x : 0.f; s.b.y = ok ? s.b.y : 0.f; s.b.z = ok ? s.b.z : 0.f; s.b.w = ok ? s.b.w : 0.f;
}
__device__ __forceinline__ void stage_mask(Stage<unsigned short>& s, bool ok) {
    typedef __attribute__((ext_vector_type(4))) int i32x4;
    i32x4 v = __builtin_bit_cast(i32x4, s.v);
    v[0] = ok ? v[0] : 0; v[1] = ok ? v[1] : 0; v[2] = ok ? v[2] : 0; v[3] = ok ? v[3] : 0;
    s.v = __builtin_bit_cast(bf16x8, v);
}
__device__ __forceinline__ void split1(float x, short& hi, short& lo) {
    const unsigned short h = f2bf(x);
    hi = (short)h;
    lo = (short)f2bf(x - bf2f(h));
}
__device__ __forceinline__ void stage_split(const Stage<float>& s, bf16x8& hi, bf16x8& lo) {
    short h, l;
    split1(s.a.x, h, l); hi[0] = h; lo[0] = l;
    split1(s.a.y, h, l); hi[1] = h; lo[1] = l;
    split1(s.a.z, h, l); hi[2] = h; lo[2] = l;
    split1(s.a.w, h, l); hi[3] = h; lo[3] = l;
    split1(s.b.x, h, l); hi[4] = h; lo[4] = l;
    split1(s.b.y, h, l); hi[5] = h; lo[5] = l;
    split1(s.b.z, h, l); hi[6] = h; lo[6] = l;
    split1(s.b.w, h, l); hi[7] = h; lo[7] = l;
}
__device__ __forceinline__ void stage_split(const Stage<unsigned short>& s, bf16x8& hi, bf16x8& lo) {
    hi = s.v;
    lo = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
}
template <bool F16>
__device__ __forceinline__ bf16x8 stage_round(const Stage<float>& s) {
    bf16x8 r;
    if constexpr (F16) {
        r[0] = (short)f2h(s.a.x); r[1] = (short)f2h(s.a.y); r[2] = (short)f2h(s.a.z); r[3] = (short)f2h(s.a.w);
        r[4] = (short)f2h(s.b.x); r[5] = (short)f2h(s.b.y); r[6] = (short)f2h(s.b.z); r[7] = (short)f2h(s.b.w);
    } else {
        r[0] = (short)f2bf(s.a.x); r[1] = (short)f2bf(s.a.y); r[2] = (short)f2bf(s.a.z); r[3] = (short)f2bf(s.a.w);
        r[4] = (short)f2bf(s.b.x); r[5] = (short)f2bf(s.b.y); r[6] = (short)f2bf(s.b.z); r[7] = (short)f2bf(s.b.w);
    }
    return r;
}
template <bool F16>
__device__ __forceinline__ bf16x8 stage_round(const Stage<unsigned short>& s) { return s.v; }   // 16-bit operands pass through

// F16: the 16-bit operands are fp16 (SKIMI_PREC_F16: fp32 inputs are rounded to fp16 while staged) and the matrix
// instruction is v_mfma_f32_32x32x16_f16; otherwise bf16.  NSPLIT 3 (bf16x3) is bf16 only.
template <int BM, int BN, int BK, int NSPLIT, typename TA, typename TW, int DEPTH, bool F16 = false>
__global__ __launch_bounds__(256) void gemm_kernel(const GemmArgs p) {
    constexpr int CPR = BK / 8;        // 16-B chunks per LDS row
    constexpr int RB = BK * 2;         // LDS row bytes
    constexpr int RPB = 256 / RB;      // LDS rows per 256-B bank row
    constexpr int A_IT = BM * CPR / 256;
    constexpr int W_IT = BN * CPR / 256;
    constexpr int NPL = (NSPLIT == 3) ? 2 : 1;   // planes per operand (hi, lo)
    constexpr int A_PLANE = BM * RB;
    constexpr int W_PLANE = BN * RB;
    constexpr int BUF = NPL * (A_PLANE + W_PLANE);
    constexpr int WM = BM / 2, WN = BN / 2, MT = WM / 32, NT = WN / 32;

    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;

    // workgroup -> (K split, tile), XCD-contiguous (gfx950.h) over the 2-D grid in launch order (x fastest, then
    // y).  Each XCD takes a contiguous run of the split-major order (split, tile): with split-K it owns whole K
    // ranges, so every byte of W and of A is pulled through ONE L2 instead of through the L2 of every XCD that
    // holds a tile of that row / column (measured on the B = 1 lifter convs: FETCH_SIZE 51 MB for 14.5 MB of
    // operands before).
    int id, ks;
    {
        const int ntile = p.ntm * p.ntn;
        const int nblk = ntile * (int)gridDim.y;
        const int lin = (int)blockIdx.y * (int)gridDim.x + (int)blockIdx.x;
        const int ord = xcd_contiguous_id(lin, nblk);
        ks = ord / ntile;
        id = ord - ks * ntile;
    }
    const int tm = id / p.ntn, tn = id - tm * p.ntn;
    const int m0 = tm * BM, n0 = tn * BN;

    const int kb = ks * p.k_per_split;
    const int ke = min(p.K, kb + p.k_per_split);
    const int nkt = (ke - kb + BK - 1) / BK;

    // ---- per-thread staging coordinates ----
    int a_r[A_IT], a_c[A_IT];
    bool a_ok[A_IT];
    long a_base[A_IT];            // plain: row base (elements); conv: window's top-left pixel + chunk (elements)
    int a_iy0[A_IT], a_ix0[A_IT];
#pragma unroll
    for (int i = 0; i < A_IT; ++i) {
        int q = i * 256 + tid;
        a_r[i] = q / CPR;
        a_c[i] = q % CPR;
        int m = m0 + a_r[i];
        a_ok[i] = m < p.M;
        if (!a_ok[i]) m = p.M - 1;
        if (p.a_mode == 0) {
            a_base[i] = (long)m * p.lda;
            a_iy0[i] = a_ix0[i] = 0;
        } else {
            int ohw = p.OH * p.OW;
            int img = m / ohw;
            int rem = m - img * ohw;
            int oy = rem / p.OW;
            int ox = rem - oy * p.OW;
            a_iy0[i] = oy * p.stride - p.pad;
            a_ix0[i] = ox * p.stride - p.pad;
            // window's top-left pixel + this lane's chunk; the tap / channel part is wave-uniform (per K-tile)
            a_base[i] = (((long)img * p.cH + a_iy0[i]) * p.cW + a_ix0[i]) * p.lda + a_c[i] * 8;
        }
    }
    int w_r[W_IT], w_c[W_IT];
    bool w_ok[W_IT];
    long w_base[W_IT];
#pragma unroll
    for (int i = 0; i < W_IT; ++i) {
        int q = i * 256 + tid;
        w_r[i] = q / CPR;
        w_c[i] = q % CPR;
        int n = n0 + w_r[i];
        w_ok[i] = n < p.N;
        if (!w_ok[i]) n = p.N - 1;
        w_base[i] = (long)n * p.ldw;
    }

    // DEPTH register staging sets = global-load prefetch distance in K-tiles.  DEPTH 1 is the
    // plain double-buffered loop; skinny problems (few MFMAs per tile) are load-latency-bound and
    // run with DEPTH 4 so that three tiles of loads are always in flight.
    Stage<TA> sa[DEPTH][A_IT];
    Stage<TW> sw[DEPTH][W_IT];
    unsigned okmask[DEPTH];

    f32x16 acc[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int l31 = lane & 31, lh = lane >> 5;

#define LDS_OFF(r, c) ((r) * RB + ((((c) ^ (((r) / RPB) % CPR))) << 4))

// issue the global loads of K-tile T into register set SET (unconditional loads, clamped address)
#define ISSUE_TILE(T, SET)                                                                              \
    {                                                                                                   \
        const int k0 = kb + (T) * BK;                                                                   \
        int tap_dy = 0, tap_dx = 0, cin0 = k0;                                                          \
        if (p.a_mode != 0) {                                                                            \
            int tap = k0 / p.cC;                                                                        \
            cin0 = k0 - tap * p.cC;                                                                     \
            if (p.a_mode == 2) { /* slice-major K: k = ((c / 32) * taps + tap) * 32 + c % 32 */         \
                const int u = k0 >> 5, nt = p.KH * p.KW;                                                \
                const int cs = u / nt;                                                                  \
                tap = u - cs * nt;                                                                      \
                cin0 = cs * 32 + (k0 & 31);                                                             \
            }                                                                                           \
            int ky = tap / p.KW;                                                                        \
            int kx = tap - ky * p.KW;                                                                   \
            tap_dy = ky * p.dil;                                                                        \
            tap_dx = kx * p.dil;                                                                        \
        }                                                                                               \
        unsigned okm = 0;                                                                               \
        const long tap_off = ((long)tap_dy * p.cW + tap_dx) * p.lda + cin0;  /* wave-uniform */         \
        _Pragma("unroll") for (int i = 0; i < A_IT; ++i) {                                              \
            const int kk = k0 + a_c[i] * 8;                                                             \
            bool ok = a_ok[i] && kk < ke;                                                               \
            long off;                                                                                   \
            if (p.a_mode == 0) {                                                                        \
                off = a_base[i] + kk;                                                                   \
            } else {                                                                                    \
                int iy = a_iy0[i] + tap_dy, ix = a_ix0[i] + tap_dx;                                     \
                ok = ok && iy >= 0 && iy < p.cH && ix >= 0 && ix < p.cW;                                \
                off = a_base[i] + tap_off;                                                              \
            }                                                                                           \
            stage_load(sa[SET][i], reinterpret_cast<const TA*>(p.A) + (ok ? off : 0));                  \
            okm |= ok ? (1u << i) : 0u;                                                                 \
        }                                                                                               \
        _Pragma("unroll") for (int i = 0; i < W_IT; ++i) {                                              \
            const int kk = k0 + w_c[i] * 8;                                                             \
            const bool ok = w_ok[i] && kk < ke;                                                         \
            stage_load(sw[SET][i], reinterpret_cast<const TW*>(p.W) + (ok ? (w_base[i] + kk) : 0));     \
            okm |= ok ? (1u << (16 + i)) : 0u;                                                          \
        }                                                                                               \
        okmask[SET] = okm;                                                                              \
    }

// park register set SET (K-tile T) in LDS buffer T & 1, splitting / rounding on the way
#define PARK_TILE(T, SET)                                                                               \
    {                                                                                                   \
        char* base = smem + ((T) & 1) * BUF;                                                            \
        _Pragma("unroll") for (int i = 0; i < A_IT; ++i) {                                              \
            const int o = LDS_OFF(a_r[i], a_c[i]);                                                      \
            stage_mask(sa[SET][i], (okmask[SET] >> i) & 1u);                                            \
            if (NSPLIT == 3) {                                                                          \
                bf16x8 hi, lo;                                                                          \
                stage_split(sa[SET][i], hi, lo);                                                        \
                *reinterpret_cast<bf16x8*>(base + o) = hi;                                              \
                *reinterpret_cast<bf16x8*>(base + A_PLANE + o) = lo;                                    \
            } else {                                                                                    \
                *reinterpret_cast<bf16x8*>(base + o) = stage_round<F16>(sa[SET][i]);                         \
            }                                                                                           \
        }                                                                                               \
        char* wbw = base + NPL * A_PLANE;                                                               \
        _Pragma("unroll") for (int i = 0; i < W_IT; ++i) {                                              \
            const int o = LDS_OFF(w_r[i], w_c[i]);                                                      \
            stage_mask(sw[SET][i], (okmask[SET] >> (16 + i)) & 1u);                                     \
            if (NSPLIT == 3) {                                                                          \
                bf16x8 hi, lo;                                                                          \
                stage_split(sw[SET][i], hi, lo);                                                        \
                *reinterpret_cast<bf16x8*>(wbw + o) = hi;                                               \
                *reinterpret_cast<bf16x8*>(wbw + W_PLANE + o) = lo;                                     \
            } else {                                                                                    \
                *reinterpret_cast<bf16x8*>(wbw + o) = stage_round<F16>(sw[SET][i]);                          \
            }                                                                                           \
        }                                                                                               \
    }

    // prologue: DEPTH tiles of loads in flight, tile 0 parked
#pragma unroll
    for (int d = 0; d < DEPTH; ++d)
        if (d < nkt) ISSUE_TILE(d, d)
    if (nkt > 0) PARK_TILE(0, 0)
    __syncthreads();

    // steady state, unrolled by DEPTH so every register-set index is a compile-time constant:
    // iteration kt re-fills set kt % DEPTH (its tile was parked one iteration ago) with tile
    // kt + DEPTH, runs the MFMAs of tile kt from LDS, then parks tile kt + 1.
    for (int kt0 = 0; kt0 < nkt; kt0 += DEPTH) {
#pragma unroll
        for (int j = 0; j < DEPTH; ++j) {
            const int kt = kt0 + j;
            if (kt < nkt) {
                if (kt + DEPTH < nkt) ISSUE_TILE(kt + DEPTH, j)
                {
                    // ---- MFMAs of tile kt ----
                    const char* ab = smem + (kt & 1) * BUF;
                    const char* wb = ab + NPL * A_PLANE;
#pragma unroll
                    for (int s = 0; s < BK / 16; ++s) {
                        bf16x8 a_hi[MT], w_hi[NT], a_lo[MT], w_lo[NT];
#pragma unroll
                        for (int i = 0; i < MT; ++i) {
                            const int row = wr * WM + i * 32 + l31;
                            const int o = LDS_OFF(row, 2 * s + lh);
                            a_hi[i] = *reinterpret_cast<const bf16x8*>(ab + o);
                            if (NSPLIT == 3) a_lo[i] = *reinterpret_cast<const bf16x8*>(ab + A_PLANE + o);
                        }
#pragma unroll
                        for (int jj = 0; jj < NT; ++jj) {
                            const int row = wc * WN + jj * 32 + l31;
                            const int o = LDS_OFF(row, 2 * s + lh);
                            w_hi[jj] = *reinterpret_cast<const bf16x8*>(wb + o);
                            if (NSPLIT == 3) w_lo[jj] = *reinterpret_cast<const bf16x8*>(wb + W_PLANE + o);
                        }
#pragma unroll
                        for (int i = 0; i < MT; ++i)
#pragma unroll
                            for (int jj = 0; jj < NT; ++jj) {
                                if (NSPLIT == 3) {
                                    acc[i][jj] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_lo[i], w_hi[jj], acc[i][jj], 0, 0, 0);
                                    acc[i][jj] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_hi[i], w_lo[jj], acc[i][jj], 0, 0, 0);
                                }
                                acc[i][jj] = mfma_32x32x16<F16>(a_hi[i], w_hi[jj], acc[i][jj]);
                            }
                    }
                }
                if (kt + 1 < nkt) PARK_TILE(kt + 1, (j + 1) % DEPTH)
                __syncthreads();
            }
        }
    }
#undef ISSUE_TILE
#undef PARK_TILE
#undef LDS_OFF

    // ---- split-K: add the raw partial sums straight from the accumulator layout: one register
    // of a 32x32 tile is 2 rows x 32 consecutive columns = two 128-B segments per wave-instruction,
    // the shape global float atomics run at full rate in (MI355X_MICROARCH.md, global float atomics)
    if (p.splitk > 1) {
        // splitk_ordered (every mode unless SKIMI_SPLITK_ATOMIC): every split stores its partial tile into its own plane of the slab and
        // the epilogue adds the planes in split order -- the same bits on every run; otherwise one plane and atomics
        float* dst = p.partial + (p.splitk_ordered ? (long)ks * p.M * p.N : 0l);
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int j = 0; j < NT; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int m = m0 + wr * WM + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                    const int n = n0 + wc * WN + j * 32 + l31;
                    if (m < p.M && n < p.N) {
                        if (p.splitk_ordered) dst[(long)m * p.N + n] = acc[i][j][r];
                        else atomicAdd(dst + (long)m * p.N + n, acc[i][j][r]);
                    }
                }
        return;
    }

    // ---- epilogue: accumulators -> per-wave LDS tile -> row-contiguous 16-B stores ----
    // (the K loop ended on a barrier, so the staging buffers are free)
    float* stg = reinterpret_cast<float*>(smem) + wave * (WM * WN);
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                stg[(i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh) * WN + j * 32 + l31] = acc[i][j][r];
    __syncthreads();
    constexpr int LPR = WN / 4;          // lanes per row
    constexpr int RPI = 64 / LPR;        // rows per wave-instruction
    const int col_l = 4 * (lane % LPR);
    const int n = n0 + wc * WN + col_l;
#pragma unroll 1
    for (int it = 0; it < WM / RPI; ++it) {
        const int row_l = it * RPI + lane / LPR;
        const int m = m0 + wr * WM + row_l;
        if (m >= p.M || n >= p.N) continue;
        const float4 v = *reinterpret_cast<const float4*>(&stg[row_l * WN + col_l]);
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

// second pass of a split-K launch: partial[M,N] -> epilogue -> out
__global__ __launch_bounds__(256) void gemm_splitk_epilogue(const GemmArgs p) {
    const long total = (long)p.M * p.N;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const int m = (int)(idx / p.N);
        const int n = (int)(idx - (long)m * p.N);
        const RowMap rm = row_map(p, m);
        float v = p.partial[idx];
        // leave the slab zeroed for the next split-K launch that shares it (no memset per launch)
        p.partial[idx] = 0.f;
        if (p.splitk_ordered) {   // planes 1 .. splitk-1, added in split order (fixed summation order: run-to-run identical)
            for (int sk = 1; sk < p.splitk; ++sk) {
                float* q = p.partial + (long)sk * total + idx;
                v += *q;
                *q = 0.f;
            }
        }
        store_one(p, rm, n, v);
    }
}

template <int BM, int BN, int BK, int NSPLIT, typename TA, typename TW, bool F16 = false>
static int launch_cfg(const GemmArgs& a, hipStream_t st) {
    // 64 x 64 tiles serve the skinny, load-latency-bound shapes: prefetch 4 K-tiles deep
    constexpr int DEPTH = (BM == 64 && BN == 64) ? 4 : 1;
    constexpr int NPL = (NSPLIT == 3) ? 2 : 1;
    constexpr size_t lds = 2ull * NPL * (BM + BN) * BK * 2;
    auto kfn = gemm_kernel<BM, BN, BK, NSPLIT, TA, TW, DEPTH, F16>;
    SKIMI_LDS_OPT_IN(kfn, lds, "gemm");
    dim3 grid(a.ntm * a.ntn, a.splitk);
    hipLaunchKernelGGL(kfn, grid, dim3(256), lds, st, a);
    SKIMI_LAUNCH_CHECK();
    return SKIMI_OK;
}

static thread_local int tl_gemm_path = 0;
void set_gemm_path(int family, int tile, int mfma, int epi, int splitk) {
    tl_gemm_path = family | (tile << 4) | (mfma << 8) | (epi << 12) | (splitk << 16);
}
int gemm_last_path() { return tl_gemm_path; }

// the descriptor checks of skimi_gemm; their order decides which message a bad descriptor gets
static int check_desc(const skimi_gemm_desc* d) {
    SKIMI_CHECK_ARG(d != nullptr, "skimi_gemm: null descriptor");
    SKIMI_CHECK_ARG(d->M > 0 && d->N > 0 && d->K > 0, "skimi_gemm: empty shape M=%d N=%d K=%d", d->M, d->N, d->K);
    SKIMI_CHECK_ARG(d->K % 8 == 0, "skimi_gemm: K=%d must be a multiple of 8", d->K);
    SKIMI_CHECK_ARG(d->A && d->W && (d->out || d->out_records), "skimi_gemm: null buffer");
    const bool fold = d->a_mode == 3 || d->store_mode == 2;
    if (fold) {
        SKIMI_CHECK_ARG(d->a_mode == 3 && d->store_mode == 2, "skimi_gemm: a_mode 3 and store_mode 2 come together");
        SKIMI_CHECK_ARG(d->cC > 0 && d->cC % 32 == 0 && d->K == 4 * d->cC && (long)d->cN * d->cH * d->cW == d->M &&
                            d->ps_s >= 2 && d->N == d->ps_C && d->N % 32 == 0 && d->lda >= d->cC,
                        "skimi_gemm: bad phase-folded geometry (K = 4 cC, M = cN cH cW, N = ps_C, ps_s >= 2)");
        SKIMI_CHECK_ARG(gemm_x3dma_eligible(d),
                        "skimi_gemm: the phase-folded ConvTranspose + 3x3 conv runs on the 256-column LDS-DMA bf16x3 kernel only "
                        "(W_split, the 9-class bias table, fp32 out / records, ReLU or no activation, ps_C > 128, cW >= 2, a "
                        "chip's worth of tiles)");
    }
    if (d->out_records) {
        SKIMI_CHECK_ARG(d->N % 32 == 0 && (d->store_mode == 0 || fold) && d->out_rows_per_batch == 0 && d->out_row_off == 0 &&
                            d->out2 == nullptr && ((uintptr_t)d->out_records & 127) == 0,
                        "skimi_gemm: out_records needs N %% 32 == 0, plain output rows, no out2, 128-byte alignment");
        SKIMI_CHECK_ARG(d->out || d->out_dtype == SKIMI_F32, "skimi_gemm: records-only output is written from fp32 results");
        SKIMI_CHECK_ARG(d->prec == SKIMI_PREC_BF16X3, "skimi_gemm: out_records is an output form of the fp32-accurate mode");
    }
    SKIMI_CHECK_ARG(d->lda % 4 == 0 && d->ldw % 8 == 0 && d->lda >= 0,
                    "skimi_gemm: lda/ldw must keep 16-B alignment (lda=%ld ldw=%ld)", (long)d->lda, (long)d->ldw);
    SKIMI_CHECK_ARG(!((d->a_dtype == SKIMI_BF16 || d->a_dtype == SKIMI_F16) && d->lda % 8 != 0), "skimi_gemm: 16-bit lda must be a multiple of 8");
    SKIMI_CHECK_ARG(d->prec == SKIMI_PREC_BF16 || d->prec == SKIMI_PREC_BF16X3 || d->prec == SKIMI_PREC_F16, "skimi_gemm: bad prec %d", d->prec);
    {   // 16-bit operands carry the format of the mode: bf16 under SKIMI_PREC_BF16 / BF16X3, fp16 under SKIMI_PREC_F16
        const int bad = d->prec == SKIMI_PREC_F16 ? SKIMI_BF16 : SKIMI_F16;
        SKIMI_CHECK_ARG(d->a_dtype != bad && d->w_dtype != bad, "skimi_gemm: prec %d does not take %s operands", d->prec,
                        bad == SKIMI_BF16 ? "bf16" : "fp16");
        SKIMI_CHECK_ARG(d->prec == SKIMI_PREC_F16 || (d->out_dtype != SKIMI_F16), "skimi_gemm: fp16 output belongs to SKIMI_PREC_F16");
        SKIMI_CHECK_ARG(d->out_dtype == SKIMI_F32 || d->out_dtype == SKIMI_BF16 || d->out_dtype == SKIMI_F16, "skimi_gemm: bad out_dtype %d", d->out_dtype);
    }
    const int BK = d->prec == SKIMI_PREC_BF16X3 ? 32 : 64;
    if (d->a_mode != 0 && !fold) {
        SKIMI_CHECK_ARG(d->cC % BK == 0, "skimi_gemm: conv gather needs cC %% %d == 0 (cC=%d)", BK, d->cC);
        SKIMI_CHECK_ARG(d->a_mode != 2 || BK == 32, "skimi_gemm: slice-major conv weights (a_mode 2) need a K-tile of 32 (fp32-accurate mode)");
        SKIMI_CHECK_ARG(d->K == d->KH * d->KW * d->cC, "skimi_gemm: K != KH*KW*cC");
        SKIMI_CHECK_ARG((long)d->cN * d->OH * d->OW == d->M, "skimi_gemm: M != cN*OH*OW");
        SKIMI_CHECK_ARG((d->OH - 1) * d->stride - d->pad + (d->KH - 1) * d->dil < d->cH + d->pad &&
                        (d->OW - 1) * d->stride - d->pad + (d->KW - 1) * d->dil < d->cW + d->pad,
                        "skimi_gemm: conv window exceeds padded input");
        SKIMI_CHECK_ARG(d->lda >= d->cC, "skimi_gemm: conv pixel stride lda < cC");
    }
    if (d->store_mode == 1) {
        SKIMI_CHECK_ARG(d->ps_s > 0 && d->ps_C > 0 && d->N == d->ps_s * d->ps_s * d->ps_C &&
                        (long)d->cN * d->cH * d->cW == d->M, "skimi_gemm: bad pixel-shuffle store geometry");
    }
    if (d->resid) SKIMI_CHECK_ARG(d->ldr >= d->N, "skimi_gemm: ldr < N");
    if (d->resid2) SKIMI_CHECK_ARG(d->ldr2 >= d->N, "skimi_gemm: ldr2 < N");
    return SKIMI_OK;
}

// the kernels' argument block: the descriptor's fields, all of K in one split, and whether the epilogue may use 16-byte
// accesses (vec4); tile counts and split-K are the planner's
static GemmArgs args_from_desc(const skimi_gemm_desc* d) {
    GemmArgs a{};
    a.M = d->M; a.N = d->N; a.K = d->K;
    a.A = d->A; a.W = d->W; a.lda = d->lda; a.ldw = d->ldw;
    a.a_mode = d->a_mode;
    a.cN = d->cN; a.cH = d->cH; a.cW = d->cW; a.cC = d->cC; a.KH = d->KH; a.KW = d->KW;
    a.stride = d->stride; a.pad = d->pad; a.dil = d->dil; a.OH = d->OH; a.OW = d->OW;
    a.bias = d->bias; a.gamma = d->gamma; a.resid = d->resid; a.ldr = d->ldr; a.resid_dtype = d->resid_dtype;
    a.resid_rpb = d->resid_rows_per_batch; a.resid_bs = d->resid_batch_stride; a.resid_off = d->resid_row_off;
    a.resid2 = d->resid2; a.ldr2 = d->ldr2;
    a.out_rpb = d->out_rows_per_batch; a.out_bs = d->out_batch_stride; a.out_off = d->out_row_off;
    a.post_act = d->post_act;
    a.act = d->act;
    a.out = d->out; a.out2 = d->out2; a.out_dtype = d->out_dtype; a.ldo = d->ldo; a.ldo2 = d->ldo2;
    a.store_mode = d->store_mode; a.ps_s = d->ps_s; a.ps_C = d->ps_C;
    a.out_rec = (unsigned short*)d->out_records;
    a.rec_row = (long)(d->N / 32) * 64;
    a.f16 = d->prec == SKIMI_PREC_F16;
    a.k_per_split = d->K;
    {
        auto al16 = [](const void* q) { return ((uintptr_t)q & 15) == 0; };
        const bool out_ok = d->out_dtype == SKIMI_F32 ? al16(d->out) : (((uintptr_t)d->out & 7) == 0);
        const bool out2_ok = !d->out2 || (d->out_dtype == SKIMI_F32 ? (((uintptr_t)d->out2 & 7) == 0) : al16(d->out2));
        a.vec4 = (d->N % 4 == 0) && (d->ldo % 4 == 0) && (!d->out2 || d->ldo2 % 4 == 0) && out_ok && out2_ok &&
                 (!d->bias || al16(d->bias)) && (!d->gamma || al16(d->gamma)) &&
                 (!d->resid || ((((uintptr_t)d->resid) & 7) == 0 && (d->resid_dtype != SKIMI_F32 || al16(d->resid)) && d->ldr % 4 == 0)) &&
                 (!d->resid2 || ((((uintptr_t)d->resid2) & 7) == 0 && (d->resid_dtype != SKIMI_F32 || al16(d->resid2)) && d->ldr2 % 4 == 0)) && (d->store_mode == 0 || d->ps_C % 4 == 0);
    }
    return a;
}

// what the in-library timer counts for a launch: 2 M N K, and A (a_cols elements per output row), W and the result once
static double desc_flops(const skimi_gemm_desc* d) { return 2.0 * d->M * (double)d->N * d->K; }
static double desc_bytes(const skimi_gemm_desc* d, int a_cols) {
    const double ea = d->a_dtype == SKIMI_F32 ? 4.0 : 2.0, ew = d->w_dtype == SKIMI_F32 ? 4.0 : 2.0,
                 eo = d->out_dtype == SKIMI_F32 ? 4.0 : 2.0;
    return ea * d->M * (double)a_cols + ew * d->N * (double)d->K + eo * d->M * (double)d->N;
}

// tile and split-K of the generic kernel: fill >= ~256 CUs
struct GenericPlan {
    int BM, BN;
    int ntm, ntn;
    int splitk, k_per_split;   // k_per_split: a multiple of BK
    bool ordered;              // splitk > 1 with one slab plane per split, added in split order by the epilogue (else atomics)
    size_t scratch_need;       // bytes of split-K scratch (0: no split)
    int tile_code;             // the tile field of skimi_gemm_last_path
};

// A pure function of its arguments.  atomic: SKIMI_SPLITK_ATOMIC (A/B timing).  Every mode otherwise: a fixed summation
// order over the K splits (one slab plane per split, added in order by the epilogue) instead of global float atomics, whose
// arrival order changes the last bits from run to run -- and, through the track head's iterations, its tracks by up to a
// fifth of a pixel.
static GenericPlan plan_generic(const skimi_gemm_desc* d, const void* scratch, size_t scratch_bytes, int force_splitk, bool atomic) {
    GenericPlan p;
    const int BK = d->prec == SKIMI_PREC_BF16X3 ? 32 : 64;
    const bool small = cdiv(d->M, 128) * cdiv(d->N, 128) < 128;
    p.BM = small ? 64 : 128;
    // narrow outputs (e.g. the DPT 128 -> 32 conv): a 128 x 64 tile halves the wasted N columns
    p.BN = (p.BM == 128 && d->N <= 64) ? 64 : p.BM;
    p.ntm = (int)cdiv(d->M, p.BM);
    p.ntn = (int)cdiv(d->N, p.BN);
    const long tiles = (long)p.ntm * p.ntn;
    int splitk = 1;
    const int nkt = (int)cdiv(d->K, BK);
    bool ordered = !atomic;
    const size_t plane = (size_t)d->M * d->N * sizeof(float);
    if (force_splitk > 0) {
        splitk = force_splitk;
        if (ordered && plane * (size_t)splitk > scratch_bytes) ordered = false;   // a pinned split count (tests) on a one-plane slab
    } else if (tiles < 192 && nkt >= 8 && scratch != nullptr && plane <= scratch_bytes) {
        splitk = (int)std::min<long>(cdiv(512, tiles), nkt / 4);
        // one plane per split: as many splits as the slab holds (fewer than two: no split at all, never atomics)
        if (ordered) splitk = (int)std::min<size_t>((size_t)splitk, scratch_bytes / plane);
        if (splitk < 1) splitk = 1;
    }
    p.k_per_split = (int)cdiv(nkt, splitk) * BK;
    p.splitk = (int)cdiv(d->K, p.k_per_split);
    p.ordered = ordered && p.splitk > 1;
    p.scratch_need = p.splitk > 1 ? plane * (p.ordered ? (size_t)p.splitk : 1) : 0;
    p.tile_code = p.BM == 64 ? 1 : p.BN == 64 ? 2 : 3;
    return p;
}

// One row of launch_generic's table: if the plan's tile and the descriptor's mode are this row's, launches the kernel
// built for the operands' element types (rc) and returns true.
template <int PREC, int BM, int BN>
static bool launch_row(const GenericPlan& pl, const skimi_gemm_desc* d, const GemmArgs& a, hipStream_t st, int& rc) {
    if (d->prec != PREC || pl.BM != BM || pl.BN != BN) return false;
    constexpr bool F16 = PREC == SKIMI_PREC_F16;
    const bool af = d->a_dtype == SKIMI_F32, wf = d->w_dtype == SKIMI_F32;
    if constexpr (PREC == SKIMI_PREC_BF16X3) {   // fp32 weights (checked by launch_generic)
        if (af) rc = launch_cfg<BM, BN, 32, 3, float, float>(a, st);
        else rc = launch_cfg<BM, BN, 32, 3, unsigned short, float>(a, st);
    } else {
        if (af && wf) rc = launch_cfg<BM, BN, 64, 1, float, float, F16>(a, st);
        else if (af) rc = launch_cfg<BM, BN, 64, 1, float, unsigned short, F16>(a, st);
        else if (wf) rc = launch_cfg<BM, BN, 64, 1, unsigned short, float, F16>(a, st);
        else rc = launch_cfg<BM, BN, 64, 1, unsigned short, unsigned short, F16>(a, st);
    }
    return true;
}

static int launch_generic(const GenericPlan& pl, const GemmArgs& a, const skimi_gemm_desc* d, hipStream_t st) {
    SKIMI_CHECK_ARG(d->prec != SKIMI_PREC_BF16X3 || d->w_dtype == SKIMI_F32, "skimi_gemm: BF16X3 needs fp32 weights");
    const int rc = prof_bracket(prof_armed(PROF_GEMM, (long)d->M), st, desc_flops(d), desc_bytes(d, d->K), [&] {
        // the kernels lie in the code object in the order of these rows: a new row goes to the end
        int r = SKIMI_ERR_ARG;
        launch_row<SKIMI_PREC_F16, 128, 64>(pl, d, a, st, r) || launch_row<SKIMI_PREC_F16, 128, 128>(pl, d, a, st, r) ||
            launch_row<SKIMI_PREC_F16, 64, 64>(pl, d, a, st, r) || launch_row<SKIMI_PREC_BF16, 128, 64>(pl, d, a, st, r) ||
            launch_row<SKIMI_PREC_BF16X3, 128, 64>(pl, d, a, st, r) || launch_row<SKIMI_PREC_BF16, 128, 128>(pl, d, a, st, r) ||
            launch_row<SKIMI_PREC_BF16, 64, 64>(pl, d, a, st, r) || launch_row<SKIMI_PREC_BF16X3, 128, 128>(pl, d, a, st, r) ||
            launch_row<SKIMI_PREC_BF16X3, 64, 64>(pl, d, a, st, r);
        return r;
    });
    if (rc != SKIMI_OK) return rc;
    if (pl.splitk > 1) {
        long total = (long)d->M * d->N;
        int blocks = (int)std::min<long>(cdiv(total, 256), 2048);
        hipLaunchKernelGGL(gemm_splitk_epilogue, dim3(blocks), dim3(256), 0, st, a);
        SKIMI_LAUNCH_CHECK();
    }
    return SKIMI_OK;
}

// scratch: caller-owned fp32 slab [M, N] for split-K partials (NULL => split-K is not used)
int gemm_dispatch(const skimi_gemm_desc* d, hipStream_t st, void* scratch, size_t scratch_bytes,
                  int force_splitk) {
    tl_gemm_path = 0;
    if (const int rc = check_desc(d)) return rc;
    GemmArgs a = args_from_desc(d);
    const bool prof = prof_armed(PROF_GEMM, (long)d->M);

    // fp32-accurate path with pre-split weight records: LDS-DMA bf16x3 kernel (gemm_x3dma.hip)
    if (force_splitk <= 0 && gemm_x3dma_eligible(d)) return gemm_x3dma_launch(a, d, st);
    // the zero page behind the records (padding taps of the consumer's gather): the LDS-DMA kernels above
    // clear it themselves, the generic kernels get a memset node
    if (d->out_records &&
        hipMemsetAsync((char*)d->out_records + (size_t)d->M * (d->N / 32) * 128, 0, 256, st) != hipSuccess) {
        set_error("hipMemsetAsync(out_records zero page) failed");
        return SKIMI_ERR_HIP;
    }
    SKIMI_CHECK_ARG(d->a_dtype != SKIMI_BF16X3_REC,
                    "skimi_gemm: A given as bf16x3 records, but the launch does not qualify for the LDS-DMA kernel "
                    "(M=%d N=%d: needs W_split, M >= 4096, N >= 96, most of a chip's worth of 256-row tiles (>= 160), a zero page behind A)", d->M, d->N);

    // large bf16 x bf16 plain-row shapes: 256x256 tiles staged by LDS-DMA (gemm256.hip)
    if (force_splitk <= 0 && gemm256_eligible(d))
        return prof_bracket(prof, st, desc_flops(d), desc_bytes(d, d->K), [&] { return gemm256_launch(a, st); });

    // 3 x 3 convolutions to 128 channels on 16-bit operands (the track head's feature extractor): halo window in LDS;
    // each of A's pixels is counted once
    if (force_splitk <= 0 && conv_win_eligible(d)) {
        set_gemm_path(SKIMI_GEMM_PATH_CONV_WIN, 0, 0, 0, 1);
        return prof_bracket(prof, st, desc_flops(d), desc_bytes(d, d->cC), [&] { return conv_win_launch(a, st); });
    }

    const GenericPlan pl = plan_generic(d, scratch, scratch_bytes, force_splitk, (int)env_once("SKIMI_SPLITK_ATOMIC", 0) != 0);
    a.ntm = pl.ntm;
    a.ntn = pl.ntn;
    a.splitk = pl.splitk;
    a.k_per_split = pl.k_per_split;
    a.splitk_ordered = pl.ordered;
    if (pl.splitk > 1) {
        if (scratch == nullptr || pl.scratch_need > scratch_bytes) {
            set_error("skimi_gemm: split-K scratch too small (%zu needed, %zu given)", pl.scratch_need, scratch_bytes);
            return SKIMI_ERR_WORKSPACE;
        }
        a.partial = (float*)scratch;
        // the split-K epilogue re-zeroes what it reads, so a caller that zeroed the slab once
        // (splitk_scratch_zeroed) pays no memset per launch
        if (!d->splitk_scratch_zeroed) SKIMI_HIP(hipMemsetAsync(scratch, 0, pl.scratch_need, st));
    }
    set_gemm_path(pl.splitk == 1 ? SKIMI_GEMM_PATH_GENERIC : pl.ordered ? SKIMI_GEMM_PATH_SPLITK_ORDERED : SKIMI_GEMM_PATH_SPLITK_ATOMIC,
                  pl.tile_code, 0, 0, pl.splitk);
    return launch_generic(pl, a, d, st);
}

}  // namespace skimi
