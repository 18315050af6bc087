// VideoPose3D TemporalModel(dense=True) at small batch: the first conv of a dense block (model.py:113-116: 2 pad + 1
// taps at dilation 1 -- 7, 19, 55, 163 taps for RF 243) as a tap-reuse WINDOW convolution, bf16x3 on
// v_mfma_f32_16x16x32_bf16 (acc += Wlo Xhi + Whi Xlo + Whi Xhi, as the rest of vp3d_stream.hip).
//
//     out[l][c] = sum_t sum_ci W[c][t][ci] x[l + t][ci]
//
// vp3d_mm_kernel (vp3d_stream.hip) gathers every tap's 16-row operand tiles from global memory: a workgroup with
// R output rows re-reads its rows once per tap, taps x the bytes of its window (43 MB per workgroup for the 163-tap
// layer at B = 1).  vp3d_conv_kernel applies the shift to the output instead and needs one accumulator set per tap,
// which does not scale past a few taps.  Here the shift is applied on the INPUT side, out of LDS: per 32-channel K
// slice, the workgroup stages the (16 RT + taps - 1)-row window of its clip's hi / lo activation records in LDS once,
// and every tap's 16 x 32 operand fragments are row offsets into that window.  One accumulator set (CT channels x
// RT row tiles) per wave.
//
// Workgroup = CT = 16 TA channels x R <= 16 RT output rows of ONE clip (row splits per clip), the whole K, no K split
// across workgroups: every output is written once, by one workgroup, in a fixed order -- no atomics, deterministic,
// and a clip's result does not depend on the batch or on the tiling (the accumulation order of an output is the same
// for every (TA, RT, msc)).  Inside (8 waves): K walks slice-major, all taps of a slice before the next slice; the
// taps of a slice go round-robin to the waves (tap t -> wave t mod 8), so each wave streams its own weight fragments
// (fragment-major records, vp3d.hip upload_frag, K = tap * C + ci: tap-major, so a wave's next tap is a fixed stride
// away) from global memory into registers, one item ahead, and reads its activation fragments out of the shared
// window.  The window is double-buffered across slices: slice s + 1 comes from global memory into registers while
// slice s is consumed and goes to LDS before the slice's barrier.  The eight K-partials meet in LDS once, then the
// epilogue of vp3d_mm_kernel (bias, ReLU, fp32 and the next layer's fragment-major records).
//
// LDS window layout, per buffer: [hi | lo][kg 0..3][NR rows][8 bf16], NR = 16 RT + taps - 1 rounded up to 16.  The
// fragment of lane (li = lane & 15, kg = lane >> 4) for row tile j at tap t is the 16 bytes at row 16 j + li + t of
// plane (h, kg): every kg plane is 16 rows of consecutive 16-byte units, and with the plane pitch NR * 16 a multiple
// of 256 bytes the four lane groups of ds_read_b128 ({0-3, 12-15, 20-27} ...: two kg planes each, MI355X_MICROARCH
// §LDS) cover 16 distinct 16-byte bank quads at EVERY tap shift -- conflict-free without a swizzle.  The staging
// writes are linear (unit u of the window -> byte 16 u), and consecutive units are consecutive 16-byte pieces of
// the fragment-major source.
#include <stdlib.h>

#include <algorithm>

#include "common.h"
#include "env.h"
#include "gfx950.h"
#include "kernels.h"

namespace skimi {

struct Vp3dWin {
    const char* wrec;     // [Npad / 16][taps * C / 32][2][4][16][8] bf16 (K order: tap-major)
    const char* xrec;     // [ceil(B * Lin / 16)][C / 32][2][4][16][8] bf16
    const float* bias;    // [N]
    float* out_f32;       // [B * Lout][ldo] or null
    char* out_rec;        // fragment-major [ceil(B * Lout / 16)][N / 32][2][4][16][8] or null (N % 32 == 0)
    int B, N, C, taps, Lin, Lout, ldo;
    int R, msc;           // output rows per workgroup (<= 16 RT), row splits per clip
    int NR;               // window rows (16 RT + taps - 1, rounded up to 16)
};

constexpr int VP3D_WIN_SU = 8;                    // staging units (16 B) per thread and slice: NR * 8 <= 512 * SU
constexpr int VP3D_WIN_MAX_NR = 64 * VP3D_WIN_SU;
constexpr int VP3D_WIN_LDS_MAX = 160 * 1024;

typedef __attribute__((ext_vector_type(8))) short v8s;

template <int TA, int RT>
__global__ __launch_bounds__(512) void vp3d_win_kernel(const Vp3dWin p) {
    constexpr int NT = TA * RT, SU = VP3D_WIN_SU;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, kg = lane >> 4;
    // tile id: contiguous per XCD, as in vp3d_mm_kernel (the row splits of a channel tile share its weight slice)
    const int id = xcd_contiguous_id();
    const int per = p.B * p.msc;
    const int ct = id / per, rem = id - ct * per;
    const int b = rem / p.msc, rs = rem - b * p.msc;
    const int c0 = ct * 16 * TA, l0 = rs * p.R;
    const int SC = p.C >> 5, T = p.taps, S = T * SC;
    const int NR = p.NR, bufb = NR * 128;

    // staging: unit u = (plane hk = h * 4 + kg) * NR + window row w -> LDS byte 16 u of the buffer; window row w is
    // clip row min(l0 + w, Lin - 1) (rows past the clip feed only output rows that are never stored).  The loads are
    // unconditional (units past the window re-read its last unit: one address per wave) so that hipcc keeps counted
    // waits; only the LDS stores are masked.
    int soff[SU];
#pragma unroll
    for (int u = 0; u < SU; ++u) {
        const int idx = min(tid + 512 * u, NR * 8 - 1);
        const int hk = idx / NR, w = idx - hk * NR;
        const int g = b * p.Lin + min(l0 + w, p.Lin - 1);
        soff[u] = ((g >> 4) * SC) * 2048 + (hk >> 2) * 1024 + (hk & 3) * 256 + (g & 15) * 16;
    }
    v8s sreg[SU];
    auto stage_load = [&](int cs) {
#pragma unroll
        for (int u = 0; u < SU; ++u) sreg[u] = *reinterpret_cast<const v8s*>(p.xrec + soff[u] + (long)cs * 2048);
    };
    auto stage_store = [&](int buf) {
#pragma unroll
        for (int u = 0; u < SU; ++u)
            if (tid + 512 * u < NR * 8) *reinterpret_cast<v8s*>(smem_raw + buf * bufb + (tid + 512 * u) * 16) = sreg[u];
    };

    const char* wb[TA];
#pragma unroll
    for (int a = 0; a < TA; ++a) wb[a] = p.wrec + ((long)(c0 / 16 + a) * S) * 2048 + lane * 16;
    auto load_w = [&](v8s (&h)[TA], v8s (&l)[TA], int t, int cs) {
        const long off = (long)(t * SC + cs) * 2048;
#pragma unroll
        for (int a = 0; a < TA; ++a) {
            h[a] = *reinterpret_cast<const v8s*>(wb[a] + off);
            l[a] = *reinterpret_cast<const v8s*>(wb[a] + off + 1024);
        }
    };

    f32x4 acc[TA][RT];
#pragma unroll
    for (int a = 0; a < TA; ++a)
#pragma unroll
        for (int j = 0; j < RT; ++j) acc[a][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int ntw = wave < T ? (T - wave + 7) >> 3 : 0;   // taps of this wave in every slice: wave, wave + 8, ...
    const int rd = (kg * NR + li) * 16;                    // this lane's fragment at row tile 0, tap 0, hi plane
    v8s ah[TA], al[TA], nh[TA], nl[TA];
    stage_load(0);
    if (ntw > 0) load_w(nh, nl, wave, 0);
    stage_store(0);
    __syncthreads();
    for (int cs = 0; cs < SC; ++cs) {
        const char* win = smem_raw + (cs & 1) * bufb + rd;
        if (cs + 1 < SC) stage_load(cs + 1);
        for (int k = 0; k < ntw; ++k) {
#pragma unroll
            for (int a = 0; a < TA; ++a) {
                ah[a] = nh[a];
                al[a] = nl[a];
            }
            // the next item's weights: the next tap of this slice, or the first tap of the next slice (at the very
            // end a redundant re-read of the last slice)
            const bool last = k + 1 == ntw;
            load_w(nh, nl, last ? wave : wave + 8 * (k + 1), last ? min(cs + 1, SC - 1) : cs);
            const int t = wave + 8 * k;
            v8s bh[RT], bl[RT];
#pragma unroll
            for (int j = 0; j < RT; ++j) {
                bh[j] = *reinterpret_cast<const v8s*>(win + (16 * j + t) * 16);
                bl[j] = *reinterpret_cast<const v8s*>(win + 64 * NR + (16 * j + t) * 16);
            }
            // term-major: no MFMA waits for the accumulator of the one before it
#pragma unroll
            for (int a = 0; a < TA; ++a)
#pragma unroll
                for (int j = 0; j < RT; ++j) acc[a][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al[a], bh[j], acc[a][j], 0, 0, 0);
#pragma unroll
            for (int a = 0; a < TA; ++a)
#pragma unroll
                for (int j = 0; j < RT; ++j) acc[a][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[a], bl[j], acc[a][j], 0, 0, 0);
#pragma unroll
            for (int a = 0; a < TA; ++a)
#pragma unroll
                for (int j = 0; j < RT; ++j) acc[a][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[a], bh[j], acc[a][j], 0, 0, 0);
        }
        if (cs + 1 < SC) stage_store((cs + 1) & 1);   // the buffer read in slice cs - 1, released by its barrier
        __syncthreads();
    }

    // the eight K-partials of every 16 x 16 tile meet in LDS (the windows are dead: the last barrier above);
    // tile n is finished by wave n mod 8, summing the partials in wave order
    f32x4* red = reinterpret_cast<f32x4*>(smem_raw);   // [8 waves][NT tiles][64 lanes]
#pragma unroll
    for (int a = 0; a < TA; ++a)
#pragma unroll
        for (int j = 0; j < RT; ++j) red[(wave * NT + a * RT + j) * 64 + lane] = acc[a][j];
    __syncthreads();
    const int lend = min(l0 + p.R, p.Lout);
    for (int n = wave; n < NT; n += 8) {
        f32x4 v = red[n * 64 + lane];
#pragma unroll
        for (int w = 1; w < 8; ++w) {
            const f32x4 u = red[(w * NT + n) * 64 + lane];
            v[0] += u[0]; v[1] += u[1]; v[2] += u[2]; v[3] += u[3];
        }
        const int a = n / RT, j = n - a * RT;
        // D[i][j]: i = channel (A row) = 4 (lane >> 4) + r, j = frame (B column) = lane & 15
        const int l = l0 + 16 * j + li;
        const int c = c0 + a * 16 + 4 * kg;
        if (l >= lend || c >= p.N) continue;
        const long m = (long)b * p.Lout + l;
        float o[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = fmaxf(v[r] + p.bias[min(c + r, p.N - 1)], 0.f);   // relu(bn(conv(x))), model.py:133
        if (p.out_f32) {
            float* op = p.out_f32 + m * p.ldo + c;
            if ((p.ldo & 3) == 0 && c + 3 < p.N) {
                *reinterpret_cast<float4*>(op) = make_float4(o[0], o[1], o[2], o[3]);
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (c + r < p.N) op[r] = o[r];
            }
        }
        if (p.out_rec) {
            bf16x4 h, lo4;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const unsigned short hb = f2bf(o[r]);
                h[r] = (short)hb;
                lo4[r] = (short)f2bf(o[r] - bf2f(hb));
            }
            char* rp = p.out_rec + ((m >> 4) * (p.N >> 5) + (c >> 5)) * 2048 + (((c & 31) >> 3) * 16 + (int)(m & 15)) * 16 + (c & 7) * 2;
            *reinterpret_cast<bf16x4*>(rp) = h;
            *reinterpret_cast<bf16x4*>(rp + 1024) = lo4;
        }
    }
}

static int win_nr(int rt, int taps) { return (int)align_up((size_t)(16 * rt + taps - 1), 16); }
static size_t win_lds(int ta, int rt, int taps) {
    return std::max<size_t>((size_t)2 * 128 * win_nr(rt, taps), (size_t)8 * ta * rt * 1024);
}

template <int TA, int RT>
static int launch_win(const Vp3dWin& p, int grid, size_t lds, hipStream_t st) {
    SKIMI_LDS_OPT_IN((vp3d_win_kernel<TA, RT>), VP3D_WIN_LDS_MAX, "vp3d_win");   // once per kernel: the largest window
    hipLaunchKernelGGL((vp3d_win_kernel<TA, RT>), dim3(grid), dim3(512), lds, st, p);
    return SKIMI_OK;
}

// SKIMI_VP3D_WINDOW=0 sends the dense blocks to the per-tap kernel (vp3d_mm_kernel) instead (A/B timing; re-read on
// every forward under SKIMI_ENV_DYNAMIC=1, so that one process can alternate the two)
bool vp3d_window_enabled() {
    return (int)env_switch("SKIMI_VP3D_WINDOW", 1) != 0;
}

// The window kernel's (TA, RT, msc) for one dense conv; plan->family = 0: no window fits the LDS, the per-tap kernel
// runs the layer.  A forced (TA = force->ct, msc = force->ms; either 0: the planner's best with the other held) passes
// the planner's feasibility conditions or is refused.
int plan_vp3d_win(int Npad, int B, int Lin, int C, int taps, const Vp3dForce* force, Vp3dPlan* plan) {
    const int Lout = Lin - taps + 1;
    const int f_ta = force ? force->ct : 0, f_msc = force ? force->ms : 0;
    if (f_ta != 0 || f_msc != 0) {
        SKIMI_CHECK_ARG(f_ta == 0 || f_ta == 1 || f_ta == 2, "vp3d_win forced plan: TA %d is neither 1 nor 2", f_ta);
        SKIMI_CHECK_ARG(f_ta == 0 || Npad % (16 * f_ta) == 0, "vp3d_win forced plan: Npad %d is not a multiple of 16 TA = %d", Npad,
                        16 * f_ta);
        SKIMI_CHECK_ARG(f_msc >= 0 && f_msc <= Lout, "vp3d_win forced plan: msc %d exceeds Lout %d", f_msc, Lout);
        if (f_msc != 0) {
            const int rt = (int)cdiv(cdiv(Lout, f_msc), 16);
            SKIMI_CHECK_ARG(rt <= 8, "vp3d_win forced plan: msc %d needs %d row tiles, at most 8 fit", f_msc, rt);
            SKIMI_CHECK_ARG(win_nr(rt, taps) <= VP3D_WIN_MAX_NR, "vp3d_win forced plan: a window of %d rows exceeds the %d staged rows",
                            win_nr(rt, taps), VP3D_WIN_MAX_NR);
            for (int ta : {1, 2})
                if (f_ta == ta)
                    SKIMI_CHECK_ARG(win_lds(ta, rt, taps) <= (size_t)VP3D_WIN_LDS_MAX,
                                    "vp3d_win forced plan: %zu bytes of LDS exceed %d", win_lds(ta, rt, taps), VP3D_WIN_LDS_MAX);
        }
    }
    // (TA, RT, msc): clocks of one workgroup on its CU -- the larger of its MFMA issue on the busiest SIMD (two waves
    // per SIMD, taps round-robin over the eight waves), its LDS reads (ds_read_b128, 4 clk each) and its global bytes
    // (weights + window staging, ~64 B/clk per CU), plus a fixed cost -- times the rounds over the 256 CUs
    const int SC = C / 32;
    const double FIXED = 4000.0;
    int bt = 0, br = 0, bm = 0;
    double best = 1e30;
    for (int ta : {1, 2}) {
        if (Npad % (16 * ta)) continue;
        if (f_ta != 0 && ta != f_ta) continue;
        const int nct = Npad / (16 * ta);
        for (int msc = 1; msc <= Lout; ++msc) {
            const int R = (int)cdiv(Lout, msc), rt = (int)cdiv(R, 16);
            if (f_msc != 0 && msc != f_msc) continue;
            if (rt > 8) continue;
            if (win_nr(rt, taps) > VP3D_WIN_MAX_NR || win_lds(ta, rt, taps) > (size_t)VP3D_WIN_LDS_MAX) continue;
            const long grid = (long)nct * B * msc;
            const double mfma = 16.0 * 3 * ta * rt * 2 * cdiv(taps, 8) * SC;
            const double lds = 4.0 * 2 * rt * taps * SC;
            const double glb = (2.0 * ta * 1024 * taps + 128.0 * win_nr(rt, taps)) * SC / 64.0;
            const double cost = (double)cdiv(grid, 256) * (std::max(mfma, std::max(lds, glb)) + FIXED);
            if (cost < best) {
                best = cost; bt = ta; br = rt; bm = msc;
            }
            if (R <= 16) break;   // more row splits only shrink R below one tile
        }
    }
    if (bt == 0) {
        SKIMI_CHECK_ARG(f_ta == 0 && f_msc == 0, "vp3d_win forced plan: no window of %d taps fits the LDS at TA %d, msc %d", taps, f_ta,
                        f_msc);
        *plan = Vp3dPlan{0, 0, 0, 0, 0, 0, 0, 0, 0};
        return SKIMI_OK;
    }
    *plan = Vp3dPlan{VP3D_FAM_WIN, 16 * bt, br, taps, 8, bm, (int)cdiv(Lout, bm), (Npad / (16 * bt)) * B * bm,
                     (int)win_lds(bt, br, taps)};
    return SKIMI_OK;
}

// One dense conv (dilation 1, `taps` taps) + BN (folded) + ReLU: records in, records (and optionally fp32) out.
int vp3d_win_launch(const void* wrec, int Npad, const void* xrec, const float* bias, float* out_f32, int ldo, void* out_rec,
                    int B, int Lin, int C, int taps, int N, hipStream_t st, const Vp3dForce* force) {
    const int Lout = Lin - taps + 1;
    SKIMI_CHECK_ARG(Lout > 0 && taps >= 1 && C % 32 == 0 && Npad % 16 == 0 && Npad >= N, "vp3d_win: bad shape");
    SKIMI_CHECK_ARG(out_rec == nullptr || N % 32 == 0, "vp3d_win: records output needs N % 32 == 0");
    Vp3dPlan pl;
    int rc = plan_vp3d_win(Npad, B, Lin, C, taps, force, &pl);
    if (rc) return rc;
    if (pl.family == 0)   // no window fits the LDS (thousands of taps): the per-tap kernel
        return vp3d_mm_launch(wrec, Npad, xrec, bias, nullptr, 0, 0, out_f32, ldo, out_rec, B, Lin, C, taps, 1, N, 1, st);
    const int bt = pl.ct / 16, br = pl.rt, bm = pl.ms;
    Vp3dWin q;
    q.wrec = (const char*)wrec; q.xrec = (const char*)xrec; q.bias = bias;
    q.out_f32 = out_f32; q.out_rec = (char*)out_rec;
    q.B = B; q.N = N; q.C = C; q.taps = taps; q.Lin = Lin; q.Lout = Lout; q.ldo = ldo;
    q.msc = bm; q.R = pl.R;
    q.NR = win_nr(br, taps);
    const int grid = pl.grid;
    const size_t lds = (size_t)pl.lds;
    vp3d_set_last_plan(pl);
    rc = SKIMI_ERR_ARG;
#define SKIMI_VP3D_WIN(TA, RT) \
    if (bt == TA && br == RT) rc = launch_win<TA, RT>(q, grid, lds, st); else
    SKIMI_VP3D_WIN(1, 1) SKIMI_VP3D_WIN(1, 2) SKIMI_VP3D_WIN(1, 3) SKIMI_VP3D_WIN(1, 4)
    SKIMI_VP3D_WIN(1, 5) SKIMI_VP3D_WIN(1, 6) SKIMI_VP3D_WIN(1, 7) SKIMI_VP3D_WIN(1, 8)
    SKIMI_VP3D_WIN(2, 1) SKIMI_VP3D_WIN(2, 2) SKIMI_VP3D_WIN(2, 3) SKIMI_VP3D_WIN(2, 4)
    SKIMI_VP3D_WIN(2, 5) SKIMI_VP3D_WIN(2, 6) SKIMI_VP3D_WIN(2, 7) SKIMI_VP3D_WIN(2, 8)
    { set_error("vp3d_win: unsupported tiling %d x %d", bt, br); }
#undef SKIMI_VP3D_WIN
    if (rc) return rc;
    SKIMI_LAUNCH_CHECK();
    return SKIMI_OK;
}

}  // namespace skimi
