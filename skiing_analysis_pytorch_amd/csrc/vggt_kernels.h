// Launch wrappers of vggt_kernels.hip (HBM-bound helpers of the VGGT forward).
#pragma once
#include "common.h"

namespace skimi {

int patch_gather_launch(const float* img, void* out, int out_dtype, int F, int H, int W, int p, int Kp,
                        hipStream_t st);
int special_tokens_launch(float* x, const float* table, int F, int S, int P, int n, int C, hipStream_t st);
int bilinear_ac_planes_launch(const float* in, unsigned short* out, int N, int h, int w, int H, int W, int C, hipStream_t st,
                              const float* tabx = nullptr, const float* taby = nullptr,
                              int slice_records = 0, void* zpage = nullptr);   // out: [N, H, W, hi C | lo C] bf16
int bilinear_ac_launch(const void* in, void* out, int dtype, int N, int h, int w, int H, int W, int C,
                       hipStream_t st, const float* tabx = nullptr, const float* taby = nullptr, int out_dtype = -1,   // out_dtype -1: the input's; SKIMI_F32 from a 16-bit map
                       const float* ln_g = nullptr, const float* ln_b = nullptr, float ln_eps = 0.f);   // C == 128, fp32 out: LayerNorm of every resized pixel in the same pass
int add_uv_pos_launch(void* x, int dtype, const float* tabx, const float* taby, int N, int H, int W, int C,
                      hipStream_t st);
// x + UV embedding (tabx NULL: x alone) -> bf16x3 records [pixel][C/32][hi 32 | lo 32] + 256 zero bytes; x is left as it is
int add_uv_pos_records_launch(const float* x, const float* tabx, const float* taby, int N, int H, int W, int C, void* rec,
                              hipStream_t st);
// ConvTranspose2d(Ci, Cm, k = s, stride = s) + 3x3 conv Cm -> Co folded per output phase (vggt_kernels.hip): weight
// records of the (s + 2)^2 phase taps ((s + 2)^2 * Co * Ci * 4 bytes, as many floats of scratch in tmp) and beta [9][Co]
int dpt_fold_pack_launch(const float* wT, const float* bT, const float* wrn, int Ci, int Cm, int Co, int s, float* tmp, void* rec,
                         float* beta, hipStream_t st);
// out [N, 2h, 2w, C] = bias + the nine taps of a 3x3 / pad 1 conv summed over T [N, h, w, 9, C], the taps' channel
// contractions on the coarse map, each resized x2 (align-corners bilinear) and shifted by its tap; C % 32 == 0
int dpt_tap_sum_launch(const float* T, const float* bias, float* out, int N, int h, int w, int C, hipStream_t st);
int permute_conv_taps_launch(const float* in, float* out, int Co, int Ci, int kh, int kw, hipStream_t st);   // -> [kh, kw, Co, Ci]
int adaln_launch(const float* xn, const float* x, const float* mod, float* out, long rows, int D, hipStream_t st);
int pose_update_launch(const float* delta, float* pred_pad, float* act_out, long rows, int first, hipStream_t st);
int dpt_out_launch(const void* in, int dtype, const float* W, const float* b, int n_out, float* pts, float* conf,
                   long npix, int mode, hipStream_t st);
int f32_to_bf16_launch(const float* in, void* out, long n, hipStream_t st);
int f32_to_f16_launch(const float* in, void* out, long n, hipStream_t st);
int permute_conv_launch(const float* in, float* out, int Co, int Ci, int kh, int kw, hipStream_t st, int slice_major = 0);
int permute_convT_launch(const float* in, float* out, int Ci, int Co, int s, hipStream_t st);
int pad_cols_launch(const float* in, float* out, long rows, int K, int Kp, hipStream_t st);
int tile_vec_launch(const float* in, float* out, int n, int reps, hipStream_t st);

// The align-corners bilinear resize as bilinear_ac_planes_kernel and the fused window staging of conv_direct.hip both
// compute it: one source of the arithmetic, its contraction switched off in the text, so that the two cannot round
// differently.  One axis: output index I of a map resized from n source samples with scale = (n - 1) / (N - 1).
struct BilinearTap {
    int i0, i1;     // the two source samples
    float l0, l1;   // their weights
};
inline __host__ __device__ BilinearTap bilinear_ac_tap(float scale, int I, int n) {
#pragma clang fp contract(off)
    const float f = scale * I;
    BilinearTap t;
    t.i0 = (int)f < n - 1 ? (int)f : n - 1;
    t.i1 = t.i0 + 1 < n - 1 ? t.i0 + 1 : n - 1;
    t.l1 = fminf(fmaxf(f - t.i0, 0.f), 1.f);
    t.l0 = 1.f - t.l1;
    return t;
}
#ifdef __HIPCC__
// one value from its four source samples (+ e, the UV embedding, where add_e) -> the bf16 hi / lo halves of the fp32 result
__device__ __forceinline__ void bilinear_ac_split(const BilinearTap& ty, const BilinearTap& tx, float p00, float p01, float p10,
                                                  float p11, bool add_e, float e, short& hi, short& lo) {
#pragma clang fp contract(off)
    float r = ty.l0 * (tx.l0 * p00 + tx.l1 * p01) + ty.l1 * (tx.l0 * p10 + tx.l1 * p11);
    if (add_e) r += e;
    const unsigned short hb = f2bf(r);
    hi = (short)hb;
    lo = (short)f2bf(r - bf2f(hb));
}
#endif

}  // namespace skimi
