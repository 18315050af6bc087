/*
 * skimi.h — C-ABI of libskimi.so, the MI355X (gfx950 / CDNA4) hot path of the
 * skiing multi-view 3D-pose pipeline.
 *
 * The reference (ChenKaiXuSan/Skiing_Analysis_PyTorch) has no FFI of its own: its
 * boundary for this path is two Python call sites,
 *     preds = self.vggt(imgs)                       vggt/vggt/infer.py:84
 *     predicted_3d_pos = model_pos(inputs_2d)       VideoPose3D/run.py:974
 * and two weight formats (flat state_dicts, vggt/vggt/infer.py:62-67 and
 * VideoPose3D/run.py:286-289).  Every entry point below is what a ctypes stub at
 * those call sites binds; each one names the reference
 * function it replaces.
 *
 * Conventions
 *   - plain pointers and sizes only; no torch / C++ types cross this boundary;
 *   - every pointer marked "dev" is a device (HBM) address, "host" a host address;
 *   - every call is asynchronous on the given hipStream_t (passed as void*; NULL =
 *     the null stream), never synchronises the host, never allocates in the launch
 *     path (handles allocate once at create/finalize time);
 *   - return value 0 = ok, negative = error; skimi_last_error() returns the text of
 *     the calling thread's last error;
 *   - activations are row-major, channels-last ("NHWC" for images / feature maps,
 *     [tokens, channels] for token streams).
 */
#ifndef SKIMI_H
#define SKIMI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SKIMI_OK 0
#define SKIMI_ERR_ARG (-1)      /* bad argument / shape mismatch */
#define SKIMI_ERR_HIP (-2)      /* HIP runtime error */
#define SKIMI_ERR_STATE (-3)    /* handle not finalized / missing weight */
#define SKIMI_ERR_WORKSPACE (-4)/* workspace too small */

/* element types of buffers that cross the ABI */
#define SKIMI_F32 0
#define SKIMI_BF16 1
#define SKIMI_BF16X3_REC 2 /* skimi_gemm_desc.a_dtype only: A already split into [hi 32 | lo 32] records */
#define SKIMI_FP8MX 3      /* skimi_gemm_fp8 out_dtype only: the result as MXFP8 (payload in out, E8M0 scales in out_scales) */
#define SKIMI_F16 4        /* IEEE binary16 (operands / activations of SKIMI_PREC_F16) */

/* arithmetic mode of the MFMA contractions
 *   SKIMI_PREC_BF16   : operands rounded to bf16, one v_mfma_f32_32x32x16_bf16 per
 *                       k-step, fp32 accumulate (the reference's GPU autocast mode,
 *                       vggt/vggt/infer.py:78-84)
 *   SKIMI_PREC_BF16X3 : operands kept in fp32 in HBM, split hi+lo into two bf16 while
 *                       staged to LDS, three MFMAs per k-step (hi*hi + hi*lo + lo*hi):
 *                       ~2^-17 relative operand error, the mode that meets the 1e-3
 *                       parity bar against the fp32 CPU reference */
#define SKIMI_PREC_BF16 0
#define SKIMI_PREC_BF16X3 1
/* SKIMI_PREC_FP8 (skimi_vggt_config.prec only; BASELINE config 5): as SKIMI_PREC_BF16, but the four Linear layers
 * (qkv, proj, fc1, fc2) of every DINOv2 / frame / global block (vggt/vggt/layers/block.py:77-98, mlp.py:34-40,
 * attention.py:50-72) run on the MXFP8 MFMA (skimi_gemm_fp8): weights quantised once at finalize, activations by
 * their producers (skimi_layernorm_mx; the attention kernel's output rows, skimi_attention_out with SKIMI_FP8MX;
 * fc1's epilogue with out_dtype SKIMI_FP8MX; skimi_quant_mx where the shape rules those out); the attention
 * products (bf16), the fp32 residual stream and the heads are unchanged. */
#define SKIMI_PREC_FP8 2
/* SKIMI_PREC_F16: the Linear layers of the DINOv2 / frame / global blocks and the patch embedding
 * (vggt/vggt/layers/block.py:77-98, mlp.py:34-40, attention.py:50-72, patch_embed.py:65-78) with fp16 operands on
 * v_mfma_f32_32x32x16_f16, fp32 accumulate: the same matrix rate as bf16 with three more mantissa bits (fp16 is the
 * reference's own autocast format on GPUs below compute capability 8, vggt/vggt/infer.py:77-82).  The operand
 * rounding of the Linears is what puts bf16 outside north_star's 1e-3 on the joints (profiles/r03_precision_ablation.md);
 * with fp16 there the joints are inside it.  LayerNorm, the attention epilogue and fc1's GELU epilogue write fp16;
 * the attention products (QK^T, PV: they average their rounding noise over all keys) keep bf16 q, k, v, P; residual
 * stream, LayerNorm, softmax and accumulation are fp32 as in every mode.  In skimi_gemm_desc: fp16 (or fp32, rounded
 * to fp16 while staged) A and W, a_dtype / w_dtype SKIMI_F16 / SKIMI_F32. */
#define SKIMI_PREC_F16 3

/* activation in the GEMM epilogue */
#define SKIMI_ACT_NONE 0
#define SKIMI_ACT_RELU 1
#define SKIMI_ACT_GELU 2   /* erf form, torch.nn.GELU() default (vggt/vggt/layers/mlp.py:26) */
#define SKIMI_ACT_SILU 3
#define SKIMI_ACT_SIGMOID 4

const char* skimi_last_error(void);
int skimi_version(void);
/* sizeof(skimi_gemm_desc) as this library was built: a binding checks its own struct against it */
int skimi_sizeof_gemm_desc(void);
/* number of HIP devices visible; does not initialise a context on any */
int skimi_device_count(void);

/* Measurement hook (bench.py roofline leg): while armed, every launch of the given kernel
 * kind (1 = bf16 flash attention with seq_k >= min_size, 2 = MFMA contraction with
 * M >= min_size) is bracketed by a hipEvent pair on its own stream.  skimi_profile_stop
 * synchronises those events and returns the summed device time, the launch count and the
 * algorithmic FLOPs / bytes of the bracketed launches. */
int skimi_profile_start(int32_t kind, int64_t min_size);
int skimi_profile_stop(double* total_ms, int64_t* launches, double* flops, double* bytes);

/* ------------------------------------------------------------------------- */
/* Generic fused contraction  out = epilogue( gather(A) . W^T )               */
/* Replaces torch.nn.Linear / Conv1d / Conv2d / ConvTranspose2d(k==s) on the  */
/* path (vggt/vggt/layers/{attention,mlp,patch_embed}.py, heads/dpt_head.py,  */
/* VideoPose3D/common/model.py:126-138).                                      */
/* ------------------------------------------------------------------------- */
typedef struct skimi_gemm_desc {
    int32_t M, N, K;          /* out rows, out cols, contraction length (K % 8 == 0) */
    const void* A;            /* dev; [rows, lda] f32 or bf16, channels-last */
    const void* W;            /* dev; [N, ldw] f32 (BF16X3) or bf16 (BF16): nn.Linear layout */
    int32_t a_dtype, w_dtype; /* SKIMI_F32 / SKIMI_BF16 (SKIMI_F16 under SKIMI_PREC_F16); a_dtype SKIMI_BF16X3_REC: see W_split */
    int64_t lda, ldw;         /* in elements */
    int32_t prec;             /* SKIMI_PREC_* */
    /* A gather: a_mode 0 = plain rows; 1 = implicit im2col of a channels-last image
     * [cN, cH, cW, cC] with a KH x KW window (tap-major K: k = (ky*KW+kx)*cC + c),
     * M = cN*OH*OW, K = KH*KW*cC, cC % BK == 0 (BK = 64 for BF16, 32 for BF16X3);
     * 2 = the same gather with slice-major K (BF16X3 only, cC % 32 == 0):
     * k = ((c / 32) * KH*KW + ky*KW + kx) * 32 + c % 32, i.e. weights [N][cC/32][KH][KW][32];
     * 3 = (with store_mode 2, BF16X3 fast path only) ConvTranspose2d(kernel == stride == ps_s) followed by a
     * bias-free 3x3 / pad 1 conv, folded into ps_s x ps_s small convs on the coarse image [cN, cH, cW, cC], one per
     * output phase (y mod ps_s, x mod ps_s): W_split and bias as written by skimi_dpt_fold_pack, M = cN*cH*cW,
     * N = ps_C output channels, K = 4*cC (the longest phase), KH / KW / stride / pad / dil / OH / OW unused */
    int32_t a_mode;
    int32_t cN, cH, cW, cC, KH, KW, stride, pad, dil, OH, OW;
    /* epilogue: v = acc + bias[n]; v = act(v); v *= gamma[n]; v += resid[m', n];
     * resid row m' = m + resid_row_off (+ (m / resid_rows_per_batch) * resid_batch_skip) */
    const float* bias;        /* dev [N] or NULL */
    const float* gamma;       /* dev [N] or NULL */
    const void* resid;        /* dev or NULL; f32 or bf16 per resid_dtype */
    int32_t resid_dtype;      /* SKIMI_F32 / SKIMI_BF16, applies to resid and resid2 */
    int64_t ldr;
    int32_t resid_rows_per_batch; /* 0 = no batching of the residual row map */
    int64_t resid_batch_stride;   /* rows between consecutive batches in resid */
    int64_t resid_row_off;
    int32_t act;
    /* then: v += resid2[m, n] (plain row m, leading dim ldr2); v = post_act(v) */
    const void* resid2;       /* dev or NULL */
    int64_t ldr2;
    int32_t post_act;
    /* store_mode 0 output row remap, same form as the residual's:
     * row = (m / out_rows_per_batch) * out_batch_stride + m % out_rows_per_batch + out_row_off
     * (out_rows_per_batch 0 = row m + out_row_off) */
    int32_t out_rows_per_batch;
    int64_t out_batch_stride;
    int64_t out_row_off;
    /* store: store_mode 0 = out[row*ldo + n]; 1 = ConvTranspose2d with kernel == stride
     * (ps_s): m = (img, iy, ix) over [cN, cH, cW], n = (a*ps_s + b)*ps_C + co,
     * out[((img*cH*ps_s + iy*ps_s + a)*cW*ps_s + ix*ps_s + b)*ldo + co];
     * 2 = (with a_mode 3) the same scatter with the phase (a, b) chosen per column tile by the kernel and n = co:
     * out is [cN, cH*ps_s, cW*ps_s, ldo], out_records (allowed here) holds cN*cH*ps_s*cW*ps_s pixel rows, bias is the
     * [9][ps_C] border-class table; fp32 out, act SKIMI_ACT_NONE / SKIMI_ACT_RELU, no gamma / residuals / out2 */
    void* out;                /* dev; f32, bf16 or fp16 */
    void* out2;               /* dev or NULL: second copy in the other dtype (same indexing, ldo2) */
    int32_t out_dtype;
    int64_t ldo, ldo2;
    int32_t store_mode, ps_s, ps_C;
    /* optional caller-owned fp32 scratch of >= M*N*4 bytes: lets skinny shapes (too few
     * output tiles to fill 256 CUs) run split-K; NULL = never split.  force_splitk > 0
     * pins the split count (tests). */
    void* splitk_scratch;
    uint64_t splitk_scratch_bytes;
    int32_t force_splitk;
    /* 1 = the caller guarantees the scratch is all zero on entry (every split-K launch leaves it
     * zeroed again), so no memset is issued; 0 = the launch zeroes what it needs first */
    int32_t splitk_scratch_zeroed;
    /* optional fast path of SKIMI_PREC_BF16X3 for large shapes (M >= 4096, N >= 96, enough 256-row
     * tiles to fill the chip): W_split = the same weights as bf16 records [N][ceil(K/32)][hi 32 | lo 32]
     * (skimi_split_records), and x3_scratch = caller-owned scratch of >= 4 bytes per element of the A
     * buffer the launch touches (rows of ceil(C/32)*32 elements) + 256, where A is split once into
     * the same records and from where both operands stream through LDS-DMA.  Both NULL, or a smaller
     * scratch = generic kernel.
     * a_dtype SKIMI_BF16X3_REC: A already IS those records (of the [rows, C] buffer the launch
     * touches; lda ignored) and x3_scratch points to >= 256 zero bytes that lie behind the records
     * within 4 GiB of A (padding taps read them); such a launch must qualify for the fast path
     * (skimi_gemm returns SKIMI_ERR_ARG otherwise). */
    const void* W_split;
    void* x3_scratch;
    uint64_t x3_scratch_bytes;
    /* dev or NULL: the result also (or, with out == NULL, only) as bf16x3 records
     * [M][ceil(N/32)][hi 32 | lo 32] followed by 256 zero bytes (4 * M * ceil(N/32) * 32 + 256 bytes,
     * 128-byte aligned; N % 32 == 0, plain output rows): the a_dtype SKIMI_BF16X3_REC operand of a
     * following contraction, written by this launch's epilogue instead of a separate split pass */
    void* out_records;
} skimi_gemm_desc;

/* fp32 [rows, C] (row stride ld elements) -> bf16 planes hi[rows, C], lo[rows, C]:
 * hi = bf16(x), lo = bf16(x - hi)  (operand form of SKIMI_PREC_BF16X3's fast path) */
int skimi_split_planes(const float* x, int64_t ld, int64_t rows, int32_t C, void* hi, void* lo, void* stream);

/* fp32 [rows, C] (row stride ld elements, C % 4 == 0) -> bf16 records [rows][ceil(C/32)][hi 32 | lo 32]
 * (4 * rows * ceil(C/32) * 32 bytes; a ragged last slice is zero-filled): the hi and lo halves of
 * a 32-element K-slice share one 128-byte line (operand form of skimi_gemm_desc.W_split) */
int skimi_split_records(const float* x, int64_t ld, int64_t rows, int32_t C, void* records, void* stream);

/* Operands of skimi_gemm_desc.a_mode 3: ConvTranspose2d(C_in, C_mid, kernel = stride = s) (weight w_T [C_in, C_mid, s, s],
 * bias b_T [C_mid] or NULL) followed by Conv2d(C_mid, C_out, 3, padding = 1, bias = False) (w_rn [C_out, C_mid, 3, 3]),
 * the pair of dpt_head.py:218-221, 273-274 (resize_layers[i], then scratch.layer{i+1}_rn), folded per output phase
 * (p, q) = (y mod s, x mod s).  Along an axis phase 0 reads coarse offsets {-1, 0}, phase s-1 {0, +1}, the others {0}:
 * (s + 2)^2 phase taps in all.  w_records: (s + 2)^2 * C_out * C_in * 4 bytes, the phases row-major, each a
 * [C_out][taps * C_in] matrix with slice-major K as bf16 records (skimi_split_records' form); beta: fp32 [9][C_out],
 * b_T seen through the 3x3 taps that stay inside the fine map, class = 3 * yc + xc with yc / xc = 0 inside, 1 first
 * row / column, 2 last.  All dev; sums in float64, rounded once to fp32.  A pack-time call: it allocates its staging
 * buffer and synchronises the stream.  C_in % 32 == 0, s >= 2. */
int skimi_dpt_fold_pack(const float* w_T, const float* b_T, const float* w_rn, int32_t C_in, int32_t C_mid, int32_t C_out,
                        int32_t s, void* w_records, float* beta, void* stream);

/* A 3x3 / padding 1 conv (C_in -> C, bias) behind an x2 align-corners bilinear upsample, its channel contraction done on
 * the COARSE map: taps [N, h, w, 9, C] fp32 holds, per coarse pixel, the nine 1x1 products W[:, :, ty, tx] . x (tap
 * t = 3 ty + tx: one skimi_gemm with the [9 C][C_in] stack of the taps as its weight), and
 *   out[n, Y, X, :] = bias + sum_t [(Y + ty - 1, X + tx - 1) inside the 2h x 2w map] . resize(taps_t)(Y + ty - 1, X + tx - 1)
 * = conv2d(interpolate(x, scale 2, bilinear, align_corners=True), W, bias, padding=1), exactly in exact arithmetic, borders
 * included.  The sampling is skimi_resize_bilinear's.  out [N, 2h, 2w, C] fp32; all dev, 16-byte aligned; C % 32 == 0. */
int skimi_dpt_tap_sum(const float* taps, const float* bias, float* out, int32_t N, int32_t h, int32_t w, int32_t C, void* stream);

int skimi_gemm(const skimi_gemm_desc* d, void* stream);

/* Which kernel the calling thread's last skimi_gemm dispatch chose (a host-side record written before the
 * launch; tests pin their cases to a kernel with it).  0 before any dispatch and after an argument error.
 *   bits  0- 3  family: SKIMI_GEMM_PATH_*
 *   bits  4- 7  generic: tile (1 = 64x64, 2 = 128x64, 3 = 128x128);
 *               gemm256: main loop (1 = two-phase 256 rows, 2 = two-phase 192 rows, 3 = ping-pong, 4 = single-stream)
 *   bits  8-11  gemm256, x3dma: MFMA shape (1 = v_mfma_f32_16x16x32, 2 = v_mfma_f32_32x32x16); 0 elsewhere
 *   bits 12-15  gemm256: compile-time epilogue (0 = shared epilogue, 1 bias -> 16-bit, 2 LayerScale + residual,
 *               3 bias + GELU -> 16-bit); 0 elsewhere
 *   bits 16-23  K splits (1 = no split-K) */
#define SKIMI_GEMM_PATH_GENERIC 1
#define SKIMI_GEMM_PATH_SPLITK_ORDERED 2
#define SKIMI_GEMM_PATH_SPLITK_ATOMIC 3
#define SKIMI_GEMM_PATH_X3DMA_WIDE 4
#define SKIMI_GEMM_PATH_X3DMA_NARROW 5
#define SKIMI_GEMM_PATH_GEMM256 6
#define SKIMI_GEMM_PATH_CONV_WIN 7
int32_t skimi_gemm_last_path(void);

/* OCP microscaling FP8 (MXFP8) operands of skimi_gemm_fp8: x [rows, K] (bf16 or fp32, row stride ldx elements,
 * 16-byte aligned rows) -> payload [rows][Kp] e4m3 bytes (Kp = K rounded up to 128, tail zero) and scales
 * [rows][Kp / 32] E8M0 bytes (value 2^(byte - 127); per 32-element block the smallest power of two with
 * amax / scale <= 448, so no element clips; 0 for an all-zero block). */
int skimi_quant_mx(const void* x, int32_t dtype, int64_t ldx, int64_t rows, int32_t K, void* payload, void* scales,
                   void* stream);
/* LayerNorm(C, affine, eps) of fp32 rows (vggt/vggt/layers/block.py:77-98's norm1 / norm2) written directly as the
 * MXFP8 operand of the following skimi_gemm_fp8: payload [rows][C], scales [rows][C / 32]; the same bytes as
 * skimi_quant_mx of the fp32 LayerNorm result.  C a multiple of 256 (<= 2048), ldx % 4 == 0. */
int skimi_layernorm_mx(const float* x, int64_t ldx, int64_t rows, int32_t C, const float* gamma, const float* beta,
                       float eps, void* payload, void* scales, void* stream);
/* out[m][n] = epilogue(sum_k A[m][k] W[n][k]) on v_mfma_scale_f32_32x32x64_f8f6f4, both operands as written by
 * skimi_quant_mx (nn.Linear layout for W: [N, K]).  Epilogue: + bias[n] (or NULL); act = SKIMI_ACT_NONE or
 * SKIMI_ACT_GELU; or, with gamma != NULL, gamma[n] * (. + bias[n]) + resid[m][n] (fp32, row stride ldr; may alias
 * out: block.py:77-98's LayerScale + residual).  out fp32 or bf16, row stride ldo; N, ldo, ldr multiples of 4.
 * out_dtype SKIMI_FP8MX (with out_scales != NULL; large shapes with the GELU epilogue only, N % 128 == 0): the
 * result is written directly in the operand form of the NEXT skimi_gemm_fp8 -- payload [M][N] bytes in out
 * (ldo = N) and scales [M][N / 32] in out_scales -- so the MLP's hidden activation never exists in bf16. */
int skimi_gemm_fp8(const void* A, const void* A_scales, const void* W, const void* W_scales, int32_t M, int32_t N,
                   int32_t K, const float* bias, int32_t act, const float* gamma, const float* resid, int64_t ldr,
                   void* out, int32_t out_dtype, int64_t ldo, void* out_scales, void* stream);

/* Direct 3x3 convolution (stride 1, pad 1) of a channels-last image to 32 output channels in the
 * fp32-accurate mode: the last conv of the DPT heads at full resolution
 * (vggt/vggt/heads/dpt_head.py:224-235, scratch.output_conv2[0]).  The input comes as the two bf16
 * planes of skimi_split_planes ([F, H, W, C] each, C % 32 == 0), the weights in the packed layout
 * that skimi_conv3x3_n32_pack makes of the reference's [32, C, 3, 3] tensor
 * (2 * 32 * C * 9 bf16).  out: fp32 [F, H, W, 32]; bias [32] or NULL; relu != 0 applies ReLU. */
int skimi_conv3x3_n32_pack(const float* w, void* packed, int32_t C, void* stream);
int skimi_conv3x3_n32(const void* in_hi, const void* in_lo, const void* packed_w, const float* bias, float* out,
                      int32_t F, int32_t H, int32_t W, int32_t C, int32_t relu, void* stream);
/* The same conv on planes whose consecutive pixels lie px_stride elements apart (px_stride >= C, px_stride % 8 == 0:
 * every 16-byte chunk of every pixel is 16-byte aligned); skimi_conv3x3_n32 is px_stride = C.  The DPT heads launch it
 * on the pixel records [pixel][hi C | lo C] of skimi_resize_bilinear_planes (slice_records == 0):
 * in_lo = in_hi + C, px_stride = 2 * C. */
int skimi_conv3x3_n32_strided(const void* in_hi, const void* in_lo, const void* packed_w, const float* bias, float* out,
                              int32_t F, int32_t H, int32_t W, int32_t C, int32_t relu, int64_t px_stride, void* stream);
/* The tail of a DPT head: skimi_resize_bilinear_planes (slice_records == 0; src [F, h, w, C] fp32 to H x W, + the UV
 * tables tabx [W, C/2], taby [H, C/2] or both NULL) followed by skimi_conv3x3_n32_strided on its records.  Where every
 * 18 x 18 window of the conv touches at most 12 x 12 source samples (and SKIMI_DPT_TAIL_FUSED is not 0) one launch
 * interpolates inside the conv and rec is not touched; otherwise the two launches run through rec (F * H * W * 2 C
 * bf16).  The same bits either way.  *fused (may be NULL) says which ran. */
int skimi_conv3x3_n32_upsampled(const float* src, int32_t h, int32_t w, const float* tabx, const float* taby,
                                const void* packed_w, const float* bias, float* out, int32_t F, int32_t H, int32_t W, int32_t C,
                                int32_t relu, void* rec, int32_t* fused, void* stream);

/* ------------------------------------------------------------------------- */
/* Image preprocessing on the device (vggt/load.py:38-183)                    */
/* ------------------------------------------------------------------------- */
/* One separable pass of Pillow's 8-bit resampler (what Image.resize(..., BICUBIC) runs on the host
 * in the reference): element (o, n, i) of `in` lives at (o * n_in + n) * inner + i; `kk` is
 * [n_out, ksize] int32 22-bit fixed-point coefficients, `bounds` [n_out, 2] = (first input index,
 * tap count), both built on the host as Pillow builds them (skiing_analysis_pytorch_amd/preprocess.py).
 * Horizontal pass of an HWC image: outer = H, inner = C; vertical pass: outer = 1, inner = W * C. */
int skimi_resample_u8(const uint8_t* in, uint8_t* out, int64_t outer, int32_t n_in, int32_t n_out, int64_t inner,
                      const int32_t* kk, const int32_t* bounds, int32_t ksize, void* stream);
/* uint8 HWC (3 channels) -> fp32 [3, OH, OW] = value / 255; output pixel (y, x) reads input pixel
 * (y + y_off, x + x_off), pixels outside the input are `fill` (centre crop / white padding). */
int skimi_u8_hwc_to_f32_chw(const uint8_t* in, int32_t H, int32_t W, float* out, int32_t OH, int32_t OW, int32_t y_off,
                            int32_t x_off, float fill, void* stream);

/* ------------------------------------------------------------------------- */
/* Row-wise ops on token streams                                              */
/* ------------------------------------------------------------------------- */
/* LayerNorm over the last dim C of x[rows, C] (optionally the concatenation of two
 * sources x and x2 of C/2 channels each: the [frame | global] intermediates of
 * vggt/vggt/models/aggregator.py:250-253).  out dtype f32 or bf16.
 * Replaces torch.nn.LayerNorm (block.py:49,66; dpt_head.py:56,223). gamma/beta may be
 * NULL (elementwise_affine=False, heads/camera_head.py:66). */
int skimi_layernorm(const float* x, const float* x2, int64_t ldx, int64_t rows, int32_t C,
                    const float* gamma, const float* beta, float eps,
                    void* out, int32_t out_dtype, int64_t ldo, void* stream);

/* q/k LayerNorm(head_dim) + 2D RoPE applied in place on a packed qkv buffer
 * [tokens, 3, heads, 64] (f32 or bf16).  pos is dev int32 [tokens, 2] (y, x);
 * rope_cos/rope_sin are dev f32 [rope_npos, 16] tables (cos/sin of pos * 1/base^(i/16),
 * built on the host as rope.py:86-117 does).  Replaces attention.py:54-58 +
 * rope.py:154-188.  qn_w/kn_w NULL = no norm; pos NULL = no rope. */
int skimi_qknorm_rope(void* qkv, int32_t dtype, int64_t tokens, int32_t heads,
                      const float* qn_w, const float* qn_b, const float* kn_w, const float* kn_b,
                      float eps, const int32_t* pos, const float* rope_cos, const float* rope_sin,
                      int32_t rope_npos, void* stream);

/* Scaled-dot-product attention, no mask, softmax scale 1/sqrt(head_dim)
 * (F.scaled_dot_product_attention, attention.py:60-61).
 * qkv: [batch*seq, 3, heads, head_dim]; out: [batch*seq, heads*head_dim], same dtype.
 * dtype bf16 + head_dim 64 runs the MFMA flash kernel; f32 runs the exact fp32 kernel; any other dtype is
 * SKIMI_ERR_ARG (in all three entries; messages name `skimi_attention:` whichever entry was called). */
int skimi_attention(const void* qkv, void* out, int32_t dtype, int32_t batch, int32_t seq,
                    int32_t heads, int32_t head_dim, void* stream);
/* The same with the output type named: out_dtype == dtype, or SKIMI_F16 with dtype SKIMI_BF16 -- the form
 * SKIMI_PREC_F16 runs (bf16 q / k / v and probabilities, the result rows rounded once to fp16: the operand of
 * the proj Linear, attention.py:62-64) -- or SKIMI_FP8MX with dtype SKIMI_BF16, head_dim 64 and an even number of
 * heads: the form SKIMI_PREC_FP8 runs, the result rows as skimi_gemm_fp8's A operand, quantised from the fp32
 * quotient: `out` = e4m3 payload [batch*seq][Kp] followed by the E8M0 scales [batch*seq][Kp/32], Kp =
 * heads*head_dim rounded up to 128 (pad columns are not written). */
int skimi_attention_out(const void* qkv, void* out, int32_t dtype, int32_t out_dtype, int32_t batch, int32_t seq,
                        int32_t heads, int32_t head_dim, void* stream);

/* The attention and qk-norm launches exactly as the VGGT block forward makes them (vggt_block.hip), for the tests:
 *
 * skimi_qknorm_rope_scaled: skimi_qknorm_rope, and where it takes the fast bf16 kernel (bf16 qkv 16-byte aligned,
 * qn_w, kn_w and pos given) q is multiplied by q_scale before its one rounding to bf16; *q_scaled (host) says whether
 * it was.  The forward passes q_scale = log2(e) / sqrt(64), the form skimi_attention_ex's q_prescaled expects.
 *
 * skimi_attention_ex: skimi_attention_out (same out_dtype rules and layouts) plus
 *   q_prescaled  bf16 q / k / v: q already carries 1/sqrt(head_dim) * log2(e) (*q_scaled of the call above);
 *                ignored for f32;
 *   x3_scratch   f32 with head_dim 64: dev scratch of at least skimi_attention_x3_scratch_bytes(batch*seq,
 *                3*heads*head_dim) bytes selects the bf16x3 kernel (hi + lo operands, three MFMAs per product);
 *                NULL or a smaller one the exact-fp32 kernel;
 *   out_records  host, may be NULL.  In: non-zero asks the bf16x3 kernel for bf16x3 records instead of f32 rows;
 *                out: whether they were written.  Records are [batch*seq][heads*head_dim/32][hi 32 | lo 32] bf16
 *                (the a_dtype SKIMI_BF16X3_REC operand of skimi_gemm) followed by a 256-byte zero page, so `out`
 *                needs batch*seq*heads*head_dim*4 + 256 bytes and 128-byte alignment; when it is not aligned the
 *                call writes f32 rows and reports 0. */
int skimi_qknorm_rope_scaled(void* qkv, int32_t dtype, int64_t tokens, int32_t heads,
                             const float* qn_w, const float* qn_b, const float* kn_w, const float* kn_b,
                             float eps, const int32_t* pos, const float* rope_cos, const float* rope_sin,
                             int32_t rope_npos, float q_scale, int32_t* q_scaled, void* stream);
int skimi_attention_ex(const void* qkv, void* out, int32_t dtype, int32_t out_dtype, int32_t batch, int32_t seq,
                       int32_t heads, int32_t head_dim, int32_t q_prescaled, void* x3_scratch,
                       uint64_t x3_scratch_bytes, int32_t* out_records, void* stream);
/* bytes of x3_scratch the bf16x3 attention kernel needs for `tokens` packed qkv rows of `row_elems` f32 each */
uint64_t skimi_attention_x3_scratch_bytes(int64_t tokens, int64_t row_elems);
/* The plan of the calling thread's last attention launch (any entry above, skimi_attention_f32_strided, or a forward,
 * which leaves its last launch's): out[0] family (1 exact f32, 2 bf16x3, 3 bf16 32 queries per wave, 4 bf16 64 queries
 * per wave; 0: none yet), [1] queries per workgroup (128, or 256 for family 4), [2] output form (0 rows in the input
 * type, 1 fp16 rows, 2 MXFP8, 3 bf16x3 records), [3] q_prescaled as honoured (0 for f32 input), [4] workgroups,
 * [5] the exact-f32 kernel's HD template argument (64 or 128; 64 for the other families), [6] bytes of dynamic LDS
 * (SKIMI_ATTN_LDSPAD), [7] 0.  A refused call leaves it as it was. */
void skimi_attention_last_plan(int32_t out[8]);

/* The LayerNorm and fp32 attention launches with every argument the forward gives them (vggt_dpt.hip's DPT heads,
 * vggt_track.hip's run_mha), for kernel-level tests.
 *
 * skimi_layernorm_ex: skimi_layernorm plus
 *   grp_rows, grp_stride, grp_off   input row gather: output row r reads input row
 *                (r / grp_rows) * grp_stride + grp_off + r % grp_rows (grp_rows = 0: row r).  The DPT heads drop the
 *                special tokens of every frame with it.  grp_rows > 0 needs grp_off >= 0 and
 *                grp_stride >= grp_off + grp_rows;
 *   in_rows      rows the input buffers hold: every row index read must be below it;
 *   out_dtype    SKIMI_F32 / SKIMI_BF16 / SKIMI_F16 with row stride ldo >= C, or SKIMI_BF16X3_REC: bf16x3 records
 *                [rows][C/32][hi 32 | lo 32] followed by a 256-byte zero page (`out` 128-byte aligned, rows * C * 4 + 256
 *                bytes; C % 256 == 0 with C/256 in {1, 2, 3, 4, 6, 8}, 16-byte aligned operands, ldx % 4 == 0; ldo unused).
 *
 * skimi_attention_f32_strided: softmax(scale q k^T) v in fp32 on four separate streams.  Element (g, head, token, d)
 * of stream s sits at s + go * s_strides[3] + gi * s_strides[2] + head * s_strides[1] + token * s_strides[0] + d with
 * g = go * batch_inner + gi (batch_inner = 0: one level, gi = g).  *_strides = {token, head, batch, outer batch} in
 * elements, every one a multiple of 4, every pointer 16-byte aligned; head_dim a multiple of 4 up to 128;
 * batch <= 65535 (a grid dimension), batch_inner > 0 divides batch. */
int skimi_layernorm_ex(const float* x, const float* x2, int64_t ldx, int64_t in_rows, int64_t rows, int32_t C,
                       const float* gamma, const float* beta, float eps, void* out, int32_t out_dtype, int64_t ldo,
                       int64_t grp_rows, int64_t grp_stride, int64_t grp_off, void* stream);
int skimi_attention_f32_strided(const float* q, const float* k, const float* v, float* out, const int64_t* q_strides,
                                const int64_t* k_strides, const int64_t* v_strides, const int64_t* o_strides,
                                int32_t batch, int32_t batch_inner, int32_t heads, int32_t seq_q, int32_t seq_k,
                                int32_t head_dim, float scale, void* stream);

/* ------------------------------------------------------------------------- */
/* VideoPose3D TemporalModel lifter  (VideoPose3D/common/model.py:79-138)     */
/* ------------------------------------------------------------------------- */
typedef struct skimi_vp3d skimi_vp3d;

/* filter_widths: e.g. {3,3,3}; causal as TemporalModel(causal=...).  Same as
 * skimi_vp3d_create_ex(..., dense = 0). */
skimi_vp3d* skimi_vp3d_create(int32_t joints_in, int32_t in_features, int32_t joints_out,
                              const int32_t* filter_widths, int32_t n_widths,
                              int32_t channels, int32_t causal);
/* dense as TemporalModel(dense=...) (model.py:113-116): block i's first conv has 2*pad_i + 1
 * taps at dilation 1 instead of filter_widths[i] taps at dilation filter_widths[0]*..*[i-1];
 * pad, causal shift, receptive field and output lengths are those of the dilated model, and
 * "layers_conv.{2(i-1)}.weight" is [channels, channels, 2*pad_i + 1]. */
skimi_vp3d* skimi_vp3d_create_ex(int32_t joints_in, int32_t in_features, int32_t joints_out,
                                 const int32_t* filter_widths, int32_t n_widths,
                                 int32_t channels, int32_t causal, int32_t dense);
void skimi_vp3d_destroy(skimi_vp3d*);
/* one state_dict entry, by its reference key name ("expand_conv.weight",
 * "layers_bn.0.running_var", "shrink.bias", ...; VideoPose3D/run.py:288-289).
 * data is a host fp32 array of n elements (num_batches_tracked is ignored). */
int skimi_vp3d_set_weight(skimi_vp3d*, const char* key, const float* host_data, int64_t n);
/* fold BatchNorm (eval mode, model.py:127,134-135) into conv weight + bias, repack
 * [Cout,Cin,k] -> [Cout,k,Cin], upload.  prec selects the MFMA mode. */
int skimi_vp3d_finalize(skimi_vp3d*, int32_t prec);
int32_t skimi_vp3d_receptive_field(const skimi_vp3d*);   /* model.py:41-48 */
size_t skimi_vp3d_workspace_bytes(const skimi_vp3d*, int32_t batch, int32_t frames_in);
/* x: dev f32 [batch, frames_in, joints_in, in_features]; out: dev f32
 * [batch, frames_in - rf + 1, joints_out, 3]  (model.py:63-77) */
int skimi_vp3d_forward(skimi_vp3d*, const float* x, float* out, int32_t batch, int32_t frames_in,
                       void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------- */
/* VGGT forward  (vggt/vggt/models/vggt.py:29-96; call site infer.py:84)      */
/* ------------------------------------------------------------------------- */
typedef struct skimi_vggt skimi_vggt;

/* Shape parameters; the defaults of the reference are VGGT() = VGGT-1B
 * (vggt.py:18-27, aggregator.py:51-70, camera_head.py:26-37, dpt_head.py:40-53,
 * track_head.py:18-29).  head_dim = embed_dim / num_heads must be 64. */
typedef struct skimi_vggt_config {
    int32_t patch_size, embed_dim, depth, num_heads, num_register_tokens;
    int32_t use_dino;          /* 1: DINOv2 ViT patch embed ("dinov2_vit*14_reg"); 0: conv patch embed */
    int32_t dino_depth, dino_heads, dino_img_size;   /* dino_img_size: side the pos_embed grid was built for */
    int32_t cam_trunk_depth, cam_heads, cam_iters;
    int32_t dpt_features, dpt_out_channels[4], dpt_layers[4];
    int32_t track_features, track_hidden, track_corr_levels, track_corr_radius, track_iters, track_depth,
        track_heads, track_virtual;
    int32_t enable_camera, enable_depth, enable_point, enable_track;
    /* MFMA mode of the patch embedding and the DINOv2 / frame / global blocks: SKIMI_PREC_BF16 (the reference's
     * autocast, infer.py:78-84), SKIMI_PREC_F16 (fp16 operands: the joints stay within 1e-3 of the fp32 path),
     * SKIMI_PREC_BF16X3 (fp32-accurate) or SKIMI_PREC_FP8 */
    int32_t prec;
    /* MFMA mode of the depth / point DPT heads, which the reference runs in fp32 (torch.cuda.amp.autocast(enabled=False),
     * vggt.py:65): BF16X3 = faithful (the default everywhere); F16 / BF16 = 16-bit operands and activations, faster and
     * less accurate (fp16: depth ~1e-3 worst-case relative, profiles/r03_head_precision.json).  The camera head is
     * fp32-accurate in every mode. */
    int32_t head_prec;
} skimi_vggt_config;

skimi_vggt* skimi_vggt_create(const skimi_vggt_config* cfg);
void skimi_vggt_destroy(skimi_vggt*);
/* one entry of the reference state_dict by key ("aggregator.frame_blocks.3.attn.qkv.weight",
 * "depth_head.scratch.refinenet1.resConfUnit1.conv1.weight", ...; infer.py:62-67).
 * data: n fp32 elements on the host (on_device = 0) or already in HBM (on_device = 1). */
int skimi_vggt_set_weight(skimi_vggt*, const char* key, const float* data, int64_t n, int32_t on_device);
/* check every key of the configured model is present with the right size, repack
 * (conv taps, bf16 copies, padded K) and release the staged fp32 copies */
int skimi_vggt_finalize(skimi_vggt*);
/* DINOv2 positional embedding for an input size other than the one the model was built for:
 * pos_embed = [1 + (H/patch)*(W/patch), embed_dim] fp32 — row 0 the class position, the rest the
 * 37x37 grid resized with bicubic + antialias exactly as interpolate_pos_encoding does
 * (vggt/vggt/layers/vision_transformer.py:180-212).  A per-resolution constant, computed once by
 * the host side (skiing_analysis_pytorch_amd/vggt.py); without it such sizes are rejected. */
int skimi_vggt_set_pos_embed(skimi_vggt*, int32_t H, int32_t W, const float* pos_embed, int32_t on_device);
size_t skimi_vggt_workspace_bytes(skimi_vggt*, int32_t B, int32_t S, int32_t H, int32_t W, int32_t n_query);
/* The RoPE position table the forward uses for `frames` frames of H x W: dev int32 [frames, P, 2] (y, x), P = 1 +
 * num_register_tokens + (H/patch)*(W/patch); patches carry (row + 1, column + 1), the special tokens (0, 0)
 * (PositionGetter, vggt/vggt/layers/rope.py:39-59, + the offset of aggregator.py:219-228).  An index path: the
 * parity tests compare it bit for bit.  Synchronous copy; builds the handle's table for this shape if needed. */
int skimi_vggt_rope_positions(skimi_vggt*, int32_t frames, int32_t H, int32_t W, int32_t* positions);

/* device output buffers (fp32); a NULL pointer skips the store (a head whose outputs are all
 * NULL is not run).  Shapes as the reference's prediction dict (vggt.py:40-53). */
typedef struct skimi_vggt_outputs {
    float* pose_enc;           /* [B, S, 9] last iteration */
    float* pose_enc_list;      /* [cam_iters, B, S, 9] */
    float* depth;              /* [B, S, H, W, 1] */
    float* depth_conf;         /* [B, S, H, W] */
    float* world_points;       /* [B, S, H, W, 3] */
    float* world_points_conf;  /* [B, S, H, W] */
    float* track;              /* [B, S, N, 2] last iteration */
    float* vis;                /* [B, S, N] */
    float* conf;               /* [B, S, N] */
    float* tokens_last;        /* [B, S, P, 2*embed_dim]: aggregated_tokens_list[-1] (tests) */
} skimi_vggt_outputs;

/* images: dev f32 [B, S, 3, H, W] in [0, 1]; query_points: dev f32 [B, N, 2] pixels or NULL.
 * Errors mirror the reference: channels != 3 cannot be expressed (the layout fixes 3);
 * H or W not a multiple of patch_size -> SKIMI_ERR_ARG (patch_embed.py:69-70).
 * Concurrency: calls of any shapes (B, S, H, W) may run at the same time on one handle from several
 * host threads, each with its own workspace and stream (the handle's per-shape position / RoPE / UV
 * tables are a keyed cache of immutable entries, built under a lock on a shape's first call). */
int skimi_vggt_forward(skimi_vggt*, const float* images, const float* query_points, int32_t B, int32_t S,
                       int32_t H, int32_t W, int32_t n_query, const skimi_vggt_outputs* out,
                       void* workspace, size_t workspace_bytes, void* stream);

/* The calling thread's last skimi_vggt_forward: the workspace bytes its sizing pass planned and the bytes its launches then
 * took from the workspace (host).  The two passes run the same code and must agree. */
int skimi_vggt_last_arena(uint64_t* planned, uint64_t* used);

/* How many DPT heads, in the calling thread's forwards so far, ran scratch.output_conv1 as nine tap contractions on
 * refinenet1's coarse map + skimi_dpt_tap_sum (the fp32-accurate depth / point heads where that GEMM fills the 256-row
 * LDS-DMA kernel; SKIMI_DPT_OC1_COARSE=0, read by skimi_vggt_create, keeps the upsample + 3x3 conv on the fine map). */
int32_t skimi_vggt_oc1_coarse_count(void);

/* ------------------------------------------------------------------------- */
/* Geometry post-processing on device                                       */
/* ------------------------------------------------------------------------- */
/* pose_enc [rows, 9] (T, quat XYZW, fov_h, fov_w) -> extrinsic [rows, 3, 4] (cam-from-world,
 * OpenCV) and intrinsic [rows, 3, 3] (may be NULL) for an H x W image.
 * Replaces pose_encoding_to_extri_intri / quat_to_mat (vggt/vggt/utils/pose_enc.py:62-124,
 * rotation.py:14-44). */
int skimi_pose_to_cameras(const float* pose_enc, int64_t rows, int32_t H, int32_t W, float* extrinsic,
                          float* intrinsic, void* stream);
/* depth [frames, H, W] + cameras -> world points [frames, H, W, 3].
 * Replaces unproject_depth_map_to_point_map (vggt/vggt/utils/geometry.py:15-117), which the
 * reference runs in NumPy on the host after a D2H copy of the dense maps (infer.py:92-104). */
int skimi_unproject_depth(const float* depth, const float* extrinsic, const float* intrinsic,
                          float* world_points, int32_t frames, int32_t H, int32_t W, void* stream);
/* DLT triangulation: K [steps, views, 3, 3], R [steps, views, 3, 3], t [steps, views, 3],
 * keypoints [steps, views, joints, 2] pixels -> joints3d [steps, joints, 3].
 * Replaces triangulate_point / triangulate_one_frame (vggt/triangulate.py:13-71) for
 * views = 2 and generalises the same linear system to more views. */
int skimi_triangulate_dlt(const float* K, const float* R, const float* t, const float* keypoints,
                          float* joints3d, int64_t steps, int32_t views, int32_t joints, void* stream);

/* Triangulation with a verdict: skimi_triangulate_dlt's solve (same inputs, same float32 joints3d), then per (step, joint)
 * the stored joint through every view's OWN camera in float64: xh = K_v (R_v X + t_v), depth [steps, views, joints] = its
 * third component, err [steps, views, joints] = ||xh / depth - keypoint|| in pixels (plain division: a non-finite result
 * stays non-finite).  em = mean over the views of err; keep [steps, joints] (u8) = every depth > 0 and em finite and
 * <= err_thresh_px and, when conf [steps, views, joints] (dev f32, NULL allowed) is given, every score >= conf_thr;
 * joints3d_clean = joints3d where kept, NaN elsewhere.  view_stats [steps, views, 4] = rmse, mean, median, max of err over
 * the joints; report [steps, 5] = rmse_px, median_err_px (of em), pos_depth_ratio, kept_ratio, kept_count; NaN entries are
 * ignored as by nanmean / nanmedian / nanmax.  2 <= views <= 8, 1 <= joints <= 32.  One launch, no synchronisation.
 * Replaces reproject_and_visualize's error dict (vggt/reproject.py:108-144, :334-341) and post_triage_single
 * (triangulation/postprocess.py:70-121); rules and the one deliberate difference: DESIGN §2 "Triage". */
int skimi_triangulate_triage(const float* K, const float* R, const float* t, const float* keypoints, const float* conf,
                             double conf_thr, double err_thresh_px, int64_t steps, int32_t views, int32_t joints,
                             float* joints3d, float* joints3d_clean, double* err, double* depth, uint8_t* keep,
                             double* view_stats, double* report, void* stream);

/* Outlier-robust triangulation over 2 <= views <= 8 views (1 <= joints <= 32): inputs as skimi_triangulate_triage.  All
 * arithmetic float64, P_v = K_v [R_v | t_v] as skimi_triangulate_dlt forms it.  Per (step, joint), independent of every other
 * (rules: DESIGN §2 "Robust triangulation"):
 *  1. view v is eligible iff both keypoint coordinates are finite and (conf NULL or (double)conf >= conf_thr); fewer than
 *     two eligible views: the joint fails.
 *  2. hypotheses: every pair a < b of eligible views in lexicographic order (<= 28), the DLT solution of those two views
 *     alone (skimi_triangulate_dlt's 4 x 4 Jacobi eigen-solve); one whose system or solution is non-finite is skipped.
 *  3. scoring of a point X in every eligible view: z_v = third component of P_v (X, 1), e_v = ||(x, y) / z - keypoint||
 *     (plain division); inlier iff z_v > 0 and e_v <= inlier_px; truncated cost = sum in view order of min(e_v, inlier_px)^2,
 *     a view with z_v <= 0 or a non-finite e_v counting inlier_px^2.
 *  4. selection: most inliers, then the smaller cost, then the earlier pair; fewer than two inliers: the joint fails.
 *  5. refit, up to three rounds: X <- DLT over the inlier set (rows of view v times w_v), scored as in 3; fewer than two
 *     inliers: the previous X and set are kept (in the first round the winning hypothesis') and the refit stops; set
 *     unchanged: stop; otherwise the new set is taken.
 *  6. refine_iters (0..32) Gauss-Newton steps on c(X) = sum over the set of w_v^2 ||pi_v(X) - keypoint_v||^2: 3 x 3 normal
 *     equations from the analytic Jacobians in view order, LDL^T without pivoting; a step is taken only if it is finite
 *     and c strictly decreases, otherwise the refinement stops.  The decrease is judged by c(X + d) - c(X) formed from the
 *     step itself (per view dr . (2 r + dr), with dr the change of the residual), not by comparing two rounded sums, which
 *     cannot see steps under ~1e-10 and would leave the stopping point to the last bits of the start; d is the step X can
 *     take in float64, (X + d) - X.  The set is not re-thresholded afterwards.
 *  7. outputs: joints3d [steps, joints, 3] f32 = X (NaN x 3 for a failed joint); err [steps, views, joints] f64 = e_v of
 *     the final X for every view with finite keypoints, eligible or not (NaN otherwise; all NaN for a failed joint);
 *     inlier_views [steps, joints] u8, bit v = view v is in the final set (0: failed); rms_px [steps, joints] f64 =
 *     sqrt(mean over the set of e_v^2), unweighted; ok [steps, joints] u8 = not failed and popcount(inlier_views) >=
 *     min_inliers (2..views) and X finite; joints3d_ok = joints3d where ok, NaN elsewhere; view_inlier_ratio [steps, views]
 *     f64 = over the joints that did not fail, the share with view v in its set (NaN when all failed); report [steps, 4]
 *     f64 = ok count, ok ratio, mean popcount over the ok joints, rms of rms_px over the ok joints (NaN-aware).
 *  8. weights: weighted == 0 or conf NULL: w_v = 1; else w_v = min(max(conf, 0), 1), non-finite -> 0
 *     (VideoPose3D/slove_rt_from_3d.py:88-95).  They act in 5 and 6 only; a set with fewer than two w_v > 0 is refitted and
 *     refined unweighted.
 * One launch for all steps, no synchronisation, no allocation, no atomics, every sum in a fixed order: results are bitwise
 * reproducible and independent of `steps` and of a step's position.  Bad arguments: SKIMI_ERR_ARG before any launch.
 * The reference has no such stage (its rigs have two cameras). */
int skimi_triangulate_robust(const float* K, const float* R, const float* t, const float* keypoints, const float* conf,
                             double conf_thr, double inlier_px, int32_t min_inliers, int32_t refine_iters, int32_t weighted,
                             int64_t steps, int32_t views, int32_t joints, float* joints3d, double* err,
                             uint8_t* inlier_views, double* rms_px, uint8_t* ok, float* joints3d_ok,
                             double* view_inlier_ratio, double* report, void* stream);

/* Person origin of dense point maps (extract_person_points and the mean its caller takes,
 * vggt/multi_view_process.py:356-395, :195-199, which run in NumPy on the host).  points: dev f32 [maps, H, W, 3];
 * boxes: dev f32 [maps, 4] = x1, y1, x2, y2 in the pixels of a src_h x src_w image.  Per map: crop as the reference
 * (scale factors and products in float64, truncation toward zero, x1 in [0, W-1], x2 in [0, W], likewise y; a box with
 * a non-finite corner is empty), valid = all three coordinates finite, median = the exact middle order statistic of the
 * valid z (even count: the float64 mean of the two middle ones), std = population standard deviation in float64 (two
 * passes), kept = |z - median| < 3 std (strict, float64), origin = float64 mean of the kept points.
 * stats: dev f64 [maps, 8] = n_box, n_valid, n_kept, median, std, origin x, y, z (NaN where undefined: median and std
 * without a valid point, the origin without a kept one).  One workgroup per map, one launch, no synchronisation; sums
 * have a fixed order, so results are bitwise reproducible.  workspace: skimi_person_workspace_bytes(maps, H, W) bytes,
 * which is 0 for this kernel shape (NULL allowed).  Rules: DESIGN §2 "Person origin". */
size_t skimi_person_workspace_bytes(int64_t maps, int32_t H, int32_t W);
int skimi_person_origin(const float* points, const float* boxes, int64_t maps, int32_t H, int32_t W, int32_t src_h,
                        int32_t src_w, void* workspace, double* stats, void* stream);
/* The camera update that follows (:201-217), one thread per step: stats [steps, views, 8] from skimi_person_origin,
 * extrinsic dev f32 [steps, views, 3, 4] -> origin_out dev f64 [steps, 3] = the float64 mean of the views' origins in
 * view order (0 if any view kept no point), t_out [steps, views, 3] = t_c + R_c origin (float64, stored as f32),
 * R_out [steps, views, 3, 3] = R_c, except at views == 2 where view 1 is turned: R_1 <- diag(-1, 1, -1) R_1 and t_1 is
 * left as it is (the reference turns it and then mirrors x and z back). */
int skimi_recenter_cameras(const double* stats, const float* extrinsic, int64_t steps, int32_t views, double* origin_out,
                           float* R_out, float* t_out, void* stream);

/* Point-to-plane ICP of two dense point maps (replaces ICP_with_bbox, vggt/multi_view_process.py:427-520, which
 * calls Open3D's estimate_normals and registration_icp on the host).  Clouds are raw dev f32 [n, 3]; the validity
 * filter runs inside: a point is kept iff its coordinates are finite and x^2 + y^2 + z^2 > 1e-12 (the reference keeps
 * ||p|| > 1e-6; the two differ only on non-finite input).  Neighbours and correspondences lie at d^2 < r^2 (float64).
 * Every sum has a fixed order: results are bitwise reproducible.  ws: device scratch of at least
 * skimi_icp_workspace_bytes(n_src, n_tgt) bytes (skimi_estimate_normals: (0, n)); nothing is allocated in a call.
 * Each call synchronises `stream` (it reads valid-point counts back; ICP reads a 6x6 system per iteration). */
size_t skimi_icp_workspace_bytes(int64_t n_src, int64_t n_tgt);
/* Radius normals of the valid points (estimate_normals(KDTreeSearchParamRadius(radius)), :487-496): neighbours of a
 * point are the valid points at d < radius, itself included; with >= 3 of them the normal is the unit eigenvector of
 * the smallest eigenvalue of their float64 covariance (cumulant form), else (0, 0, 1).  The sign is arbitrary.
 * normals_out: dev f64 [n, 3], neighbour_count_out: dev i32 [n]; an invalid point gets (0, 0, 0) and 0. */
int skimi_estimate_normals(const float* points, int64_t n, double radius, double* normals_out,
                           int32_t* neighbour_count_out, void* ws, size_t ws_bytes, void* stream);
/* For tests: the correspondence of every source point under T4x4 (host f64, row-major): the nearest valid target
 * point at d < max_dist, d^2 computed in float64 from T s (ties -> the smaller target index) -> tgt_index_out
 * (dev i32 [n_src], original target indices; -1 = none or invalid source point). */
int skimi_icp_correspondences(const float* src, int64_t n_src, const float* tgt, int64_t n_tgt, const double* T4x4,
                              double max_dist, int32_t* tgt_index_out, void* ws, size_t ws_bytes, void* stream);
/* registration_icp with TransformationEstimationPointToPlane (:498-505), target normals at normal_radius:
 * evaluate(T) -> for each iteration: solve JtJ x = -Jtr (LDLT, r = (T s - t).n, J = [T s x n ; n]), update =
 * Rz(x2) Ry(x1) Rx(x0) | x3..5 (identity without correspondences or on a non-finite solution), T = update T,
 * evaluate(T), stop when |d fitness| < rel_fitness and |d rmse| < rel_rmse.  The source is always the original
 * float32 cloud transformed by T in float64.  init4x4 (host f64, NULL = identity); T_out (host f64 [16]),
 * fitness = correspondences / valid source points, rmse = sqrt(sum d^2 / correspondences) of the last evaluation,
 * iterations = updates applied.  Fewer than 50 valid points in either cloud: identity, 0, 0, 0 iterations (:471-474). */
int skimi_icp_point_to_plane(const float* src, int64_t n_src, const float* tgt, int64_t n_tgt, double max_corr_dist,
                             double normal_radius, int32_t max_iteration, double rel_fitness, double rel_rmse,
                             const double* init4x4, double* T_out, double* fitness_out, double* rmse_out,
                             int32_t* iterations_out, void* ws, size_t ws_bytes, void* stream);

/* Bundle adjustment of one clip (run_local_ba, called at vggt/multi_view_process.py:553-564 and defined nowhere in the
 * reference): Adam (torch defaults) on the sum of the five losses of bundle_adjustment/loss.py, all in float64.
 * Inputs (dev f64): K [C,3,3], R0 [T,C,3,3], t0 [T,C,3] (world -> camera), X0 [T,J,3], x2d [T,C,J,2] pixels,
 * conf [T,C,J]; 1 <= C <= 8, 1 <= J <= 32, 1 <= T <= 2^20.  modes (host i32 [n_modes], 1..8 problems over the same
 * clip, one workgroup each): SKIMI_BA_POSE_ONLY optimises X, SKIMI_BA_POSE_CAM_T X and t, SKIMI_BA_FULL X, t and
 * w [T,C,3] with R = Exp(w) R0, w = 0 at the start.  Weights: reprojection, camera smoothness, baseline, bone length,
 * pose temporal.  Outputs (dev f64, problem-major): R_out [n_modes,T,C,3,3], t_out [n_modes,T,C,3],
 * X_out [n_modes,T,J,3]; a block a mode does not optimise is its input, bitwise.  history_out (NULL allowed):
 * [n_modes, num_iters, 6] = total, then the five weighted terms, row i at the iterate before step i+1.
 * placement: SKIMI_BA_AUTO keeps each problem's state and scratch in LDS when it fits, else in ws; _LDS / _WORKSPACE
 * force one (results are bitwise the same).  ws: at least skimi_ba_workspace_bytes(T, C, J, n_modes) bytes (unused
 * when the state is in LDS).  One launch, no synchronisation, no allocation; sums have a fixed order, so results are
 * bitwise reproducible.  Rules: DESIGN §2 "BA". */
#define SKIMI_BA_POSE_ONLY 0
#define SKIMI_BA_POSE_CAM_T 1
#define SKIMI_BA_FULL 2
#define SKIMI_BA_AUTO 0
#define SKIMI_BA_LDS 1
#define SKIMI_BA_WORKSPACE 2
size_t skimi_ba_workspace_bytes(int64_t T, int32_t C, int32_t J, int32_t modes);
int skimi_bundle_adjust(const double* K, const double* R0, const double* t0, const double* X0, const double* x2d,
                        const double* conf, int64_t T, int32_t C, int32_t J, const int32_t* modes, int32_t n_modes,
                        int32_t num_iters, double lr, double w_reproj, double w_smooth, double w_baseline,
                        double w_bone_length, double w_pose_temporal, int32_t placement, double* R_out, double* t_out,
                        double* X_out, double* history_out, void* ws, size_t ws_bytes, void* stream);

/* Camera resection from 3D points and 2D keypoints (VideoPose3D/slove_rt_from_3d.py: the lifter's joints and each view's
 * keypoints -> that camera's (R, t); the reference initialises with cv2's EPnP and refines with scipy's least_squares).
 * Inputs (dev f64): X [n_points, 3]; x2d [views, n_points, 2] pixels; conf [views, n_points] or NULL; K [views, 3, 3] or
 * NULL (inferred per problem); R0 [groups, views, 3, 3] and t0 [groups, views, 3], both or neither.  The points are cut
 * into groups = n_points / group_size consecutive groups; a problem is one (group, view) pair, solved by one workgroup
 * (one wave up to 64 points, up to 1024 threads beyond).  1 <= views <= 8, group_size <= (2^31 - 1) / 3.  All arithmetic float64.  Rules (DESIGN §2
 * "Resection", restated in tests/resect_restated.py):
 *  1. a point is used iff X is finite, its keypoint is finite in EVERY view and every view's weight >= min_conf; the weight
 *     is w = conf with non-finite -> 0, clipped to [0, 1], or 1 when conf is NULL.  Fewer than 6 used points: the problem
 *     fails (R, t, costs, statistics NaN, err NaN, n_evals 0, success 0; K_out NaN where it was to be inferred).
 *  2. K NULL: cx, cy = means of the problem's used keypoints, f = 2 max(std_x + 1e-6, std_y + 1e-6), population std in
 *     two passes.  Of K the entries (0,0), (0,1), (0,2), (1,1), (1,2) are read.
 *  3. start: R0, t0 when given; else a DLT resection: rays y = K^-1 (x, y, 1), X shifted to its centroid and scaled to mean
 *     distance sqrt(3), the 12 x 12 A^T A of the rows [Xh, 0, -u Xh], [0, Xh, -v Xh] (unweighted), the eigenvector p of its
 *     smallest eigenvalue by cyclic Jacobi to convergence, sign such that det M > 0 (M the left 3 x 3 of p as 3 x 4),
 *     R = U V^T of M = U S V^T, t = p4 3 / trace S, de-normalised.  A non-finite start (or start cost) fails the problem.
 *  4. residuals r = w (pi(K, R X + t) - x), plain division by z; loss per residual COMPONENT: SKIMI_RESECT_LINEAR, cost
 *     1/2 sum r^2; SKIMI_RESECT_SOFT_L1 with f = f_scale: z = (r / f)^2, cost 1/2 f^2 sum 2 (sqrt(1 + z) - 1), weight
 *     rho' = 1 / sqrt(1 + z).
 *  5. Levenberg-Marquardt on d = (omega, dt), R <- Exp(omega) R, t <- t + dt: H = sum rho' J^T J, g = sum rho' J^T r from
 *     the analytic Jacobian (dXc / d omega = -[R X]x), (H + lam I) d = -g by LDL^T, lam0 = 1e-3 max diag H.  A trial is
 *     accepted iff its cost c + dc is finite and <= c (1 + 1e-14), then lam <- lam / 10; else lam <- 10 lam and the trial
 *     is repeated with the same H, g.  dc is formed from the step itself (the change of each camera point, ray and
 *     residual: dr (2 r + dr) per component), not as the difference of two rounded sums.  Stop on an accepted step with
 *     ||d|| <= 1e-14 (1 + ||t||), on lam >= 1e30, or after max_evals cost evaluations.  What is counted is the start and
 *     every trial (n_evals = 1 + trials); the pass that forms H, g and c afresh at an accepted point is not, so the passes
 *     over the points are at most about twice max_evals.
 *  6. outputs (dev, problem-major [groups, views, ...]): R, t, K_out [.., 3, 3]; cost0, cost; n_evals, n_used (the masked
 *     count), success (i32: not failed and stopped by a criterion other than max_evals); err [views, n_points] f64 = the
 *     unweighted pixel error of the final pose, NaN for unused points; stats [groups, views, 3] = mean, rms, max of err
 *     over the used points.
 * One launch, no synchronisation, no allocation, no atomics; every sum has a fixed order that depends only on a point's
 * index within its group: a group's results are bitwise the same alone or among others.  ws: at least
 * skimi_resect_workspace_bytes(...) bytes, which is 0 for this kernel (NULL allowed).  Bad arguments: SKIMI_ERR_ARG before
 * any launch. */
#define SKIMI_RESECT_LINEAR 0
#define SKIMI_RESECT_SOFT_L1 1
size_t skimi_resect_workspace_bytes(int64_t n_points, int32_t views, int64_t group_size);
int skimi_resect_cameras(const double* X, const double* x2d, const double* conf, const double* K, const double* R0,
                         const double* t0, int64_t n_points, int32_t views, int64_t group_size, int32_t loss, double f_scale,
                         double min_conf, int32_t max_evals, double* R, double* t, double* K_out, double* cost0, double* cost,
                         int32_t* n_evals, int32_t* n_used, int32_t* success, double* err, double* stats, void* ws,
                         size_t ws_bytes, void* stream);
/* The pose of every view relative to view 0 of its group (slove_rt_from_3d.py:252-254), one thread per (group, view):
 * R, t dev f64 [groups, views, ...] -> R_rel = R_v R_0^T, t_rel = t_v - R_rel t_0. */
int skimi_relative_pose(const double* R, const double* t, int64_t groups, int32_t views, double* R_rel, double* t_rel,
                        void* stream);

/* Camera-and-points refinement (VideoPose3D/slove_rt_from_3d.py --refine camera_points: the lifter's joints are refined
 * together with the cameras, under an optional prior lambda_x that ties them to their start; the reference calls scipy's
 * least_squares on x0 = pack(init, X), :236, :244).  Inputs (dev f64): X [n_points, 3]; x2d [views, n_points, 2] pixels; conf
 * [views, n_points] or NULL; K [views, 3, 3] or NULL (inferred per group and view); R0 [groups, views, 3, 3] and t0 [groups,
 * views, 3], both required.  The points are cut into groups = n_points / group_size consecutive groups; a problem is one
 * group, all its views and its used points together, solved by one workgroup (one wave up to 64 points, up to 512 threads
 * beyond).  1 <= views <= 4, group_size <= (2^31 - 1) / 3.  All arithmetic float64.  Rules (DESIGN §2 "Camera + points
 * refinement", restated in tests/refine_restated.py):
 *  1. mask and weights: rule 1 of skimi_resect_cameras.  Fewer than 6 used points: the group fails (R, t, costs, statistics,
 *     moved NaN, err NaN, n_evals 0, success 0; K_out NaN where it was to be inferred; X_opt = X bit for bit).
 *  2. K NULL: rule 2 of skimi_resect_cameras, per group and view.
 *  3. start: R0, t0 and X itself.  A non-finite start (or start cost) fails the group.
 *  4. residuals: per view and used point r = w (pi(K_v, R_v X_i + t_v) - x_vi) as in skimi_resect_cameras; when lambda_x > 0
 *     three more per used point, sqrt(lambda_x) (X_i - X0_i), X0 the caller's X.  Loss per residual COMPONENT, the prior's
 *     included: SKIMI_RESECT_LINEAR or SKIMI_RESECT_SOFT_L1 with f_scale (cost, rho' as there).
 *  5. parameters: per view d_v = (omega, dt), R <- Exp(omega) R, t <- t + dt; per used point dX_i.
 *  6. step: (H + lam I) d = -g over all 6 views + 3 n parameters, H = sum rho' J^T J, g = sum rho' J^T r from the analytic
 *     Jacobian (dXc / d omega = -[R X]x, dXc / dX = R), solved exactly through the Schur complement on the points:
 *     V*_i = V_i + lam I (3 x 3 LDL^T), S = U + lam I - sum_i W_i V*_i^-1 W_i^T (6 views x 6 views), rhs = -g_c + sum_i W_i
 *     V*_i^-1 g_i, d_c = S^-1 rhs by LDL^T without pivoting, dX_i = -V*_i^-1 (g_i + W_i^T d_c).  lam0 = 1e-3 max diag H.
 *  7. a trial is accepted iff its cost c + dc is finite and <= c (1 + 1e-14), then lam <- lam / 10, floored by rule 9; else
 *     lam <- 10 lam and the trial is repeated from the stored blocks.  dc is formed from the step itself: dXc = A (omega x
 *     R X) + B omega x (omega x R X) + Exp(omega) R dX + dt with dX = (X + dX) - X, then the ray, the residual and
 *     dr (2 r + dr) as in skimi_resect_cameras; the prior's dr = sqrt(lambda_x) dX.
 *  8. stop on an accepted step with ||d|| <= 3e-8 (1 + ||(t, X)||) over all cameras and used points, on lam >= 1e30, or
 *     after max_evals cost evaluations (the start and every trial count).
 *  9. gauge: with lambda_x = 0 H is singular along the seven directions of a similarity, so lam never falls below
 *     1e-9 max diag H of the current linearisation; only costs, err and stats are determined then.
 * 10. outputs (dev): R, t, K_out [groups, views, ..]; X_opt [n_points, 3] (an unused point and a failed group keep X bit for
 *     bit; X_opt must not be X); cost0, cost, moved [groups] (moved = rms ||X_opt - X|| over the used points); n_evals,
 *     n_used, success [groups] i32; err [views, n_points] = the unweighted pixel error of the final cameras at X_opt, NaN
 *     for unused points; stats [groups, views, 3] = mean, rms, max of err.
 * One launch, no synchronisation, no allocation, no atomics; every sum has a fixed order that depends only on a point's
 * index within its group: a group's results are bitwise the same alone or among others.  ws: at least
 * skimi_refine_workspace_bytes(...) bytes = (12 + 18 views) n_points doubles: per point V_i (6), g_i (3), the trial point (3)
 * and W_iv (18 per view); 0 where n_points, views or group_size is one that skimi_refine_cameras_points refuses.  Bad arguments: SKIMI_ERR_ARG before any launch. */
size_t skimi_refine_workspace_bytes(int64_t n_points, int32_t views, int64_t group_size);
int skimi_refine_cameras_points(const double* X, const double* x2d, const double* conf, const double* K, const double* R0,
                                const double* t0, int64_t n_points, int32_t views, int64_t group_size, double lambda_x,
                                int32_t loss, double f_scale, double min_conf, int32_t max_evals, double* R, double* t,
                                double* K_out, double* X_opt, double* cost0, double* cost, int32_t* n_evals, int32_t* n_used,
                                int32_t* success, double* err, double* stats, double* moved, void* ws, size_t ws_bytes,
                                void* stream);

/* Essential matrix between two calibrated views by RANSAC over five-point hypotheses, and the pose recovered from it
 * (cv2.findEssentialMat(RANSAC, prob 0.999, threshold 1) + cv2.recoverPose as VideoPose3D/slove_rt_from_3d.py --init
 * essential and triangulation/camera_position/camera_position.py call them).  Inputs (dev f64): x2d [2, n_points, 2]
 * pixels; conf [2, n_points] or NULL; K [2, 3, 3].  The points are cut into groups = n_points / group_size consecutive
 * groups, each a problem of its own.  Four launches over all groups (mask + normalise, hypotheses, scoring, finish), no
 * host synchronisation between them, no allocation, no floating-point atomics, every floating-point sum in a fixed order.
 * All arithmetic float64.  Rules (DESIGN §2 "Essential matrix", restated in tests/essential_restated.py):
 *  1. a point is used iff both keypoints are finite and (conf NULL or both weights >= min_conf); weights as rule 1 of
 *     skimi_resect_cameras.  Normalised coordinates a = K0^-1 (x, y, 1), b = K1^-1 (x, y, 1) from K's entries (0,0),
 *     (0,1), (0,2), (1,1), (1,2): v = (y - cy) / fy, u = (x - cx - s v) / fx.  m = the used count; the used points are
 *     ranked 0 .. m - 1 in index order.  m < 5: the group fails (E, R, t, cost, confidence NaN, counts and masks 0
 *     except n_used = m, winner -1, -1, success 0).
 *  2. tau = threshold / ((fx0 + fy0 + fx1 + fy1) / 4).
 *  3. sampling: splitmix64 (s += 0x9E3779B97F4A7C15; z = s; z = (z ^ z >> 30) 0xBF58476D1CE4E5B9; z = (z ^ z >> 27)
 *     0x94D049BB133111EB; z ^= z >> 31), s0 = seed ^ ((g + group_offset) 2^32 + h) for hypothesis h of group g; the first
 *     output is discarded; each draw is the next output mod m, drawn again while that rank is in the sample already; after 64
 *     outputs (the discarded one not counted) the sample is completed with the smallest ranks not yet drawn.  No early
 *     termination: all `hypotheses` samples are solved and scored.
 *  4. five-point solver (Stewenius): rows kron(b_i, a_i) (row . vec(E) = b^T E a, E row-major), the 9 x 9 A^T A (sums in
 *     point order), cyclic Jacobi to convergence (the stopping rule of the resection's), N0..N3 = the eigenvectors of the
 *     four smallest eigenvalues in ascending order (ties: lower index), E(x, y, z) = x N0 + y N1 + z N2 + N3.  The ten
 *     cubic constraints det E = 0 and 2 E E^T E - tr(E E^T) E = 0 (row-major) over the monomials x^3, x^2 y, x y^2, y^3,
 *     x^2 z, x y z, y^2 z, x z^2, y z^2, z^3 | x^2, x y, y^2, x z, y z, z^2, x, y, z, 1 give the 10 x 20 M; B = M[:, :10]^-1
 *     M[:, 10:] by Gauss-Jordan with partial pivoting (a pivot below 1e-14 times the largest entry of its column, or a
 *     non-finite one, skips the sample); action matrix of x on the second ten monomials: rows 0..5 = -B rows 0, 1, 2, 4, 5,
 *     7; (6,0) = (7,1) = (8,3) = (9,6) = 1.  Every real eigenpair (lambda, v), v9 != 0 gives (x, y, z) = v6..8 / v9; here:
 *     Hessenberg reduction and Francis QR for the eigenvalues, the null vector of A - lambda I by elimination with full
 *     pivoting.  Each candidate is polished by a fixed number of Gauss-Newton steps on the ten constraints (10 x 3 Jacobian,
 *     3 x 3 normal equations) and kept iff max |M mon| / (1 + x^2 + y^2 + z^2)^(3/2) is finite and under a bound (steps
 *     and bound: DESIGN).  E is scaled to ||E||_F = sqrt 2; a sample's solutions are ordered by x ascending.
 *  5. Sampson e^2 = (b^T E a)^2 / ((E a)_1^2 + (E a)_2^2 + (E^T b)_1^2 + (E^T b)_2^2); inlier iff e^2 is finite and <=
 *     tau^2; cost = sum min(e^2, tau^2) in rank order, a non-finite e^2 counting tau^2.
 *  6. winner: most inliers, then the smaller cost, then the smaller hypothesis, then the smaller solution index (costs that
 *     compare neither way, NaN under a non-finite tau, count as equal).  None: the group fails.  No refit.
 *  7. E = U diag(1, 1, 0) V^T from the Jacobi eigenvectors Q of E^T E: v3 = the column k of the smallest eigenvalue, v1, v2
 *     = the columns (k + 1) % 3, (k + 2) % 3, u_i = E v_i / ||E v_i||, u3 = u1 x u2; W = [[0, -1, 0], [1, 0, 0], [0, 0, 1]];
 *     candidates (U W V^T, +u3), (U W V^T, -u3), (U W^T V^T, +u3), (U W^T V^T, -u3).
 *  8. cheirality per candidate and INLIER of the winner: the depths (z0, z1) are the least-squares solution of z0 (R a) -
 *     z1 b = -t (2 x 2 normal equations); a point passes iff both are finite, > 0 and < distance_thresh; the candidate with
 *     the most passes wins, the earlier one on a tie.
 *  9. outputs (dev): R [G, 3, 3]; t [G, 3] = baseline t^; E [G, 3, 3] = [t^]x R; inliers, pose_mask [n_points] u8 (0 for
 *     unused points); n_used, n_inliers, n_pose [G] i32; cheirality [G, 4] i32; cost [G]; winner [G, 2] i32 (hypothesis,
 *     solution); n_solutions [G] i32 (all kept candidates); confidence [G] = 1 - (1 - w^5)^H, w = n_inliers / m; success
 *     [G] i32 = a winner exists, n_inliers >= 5 and n_pose > 0.  Convention: X1 = R X0 + t, b^T E a = 0.
 * 10. 1 <= hypotheses <= 65536, 1 <= group_size <= n_points, n_points % group_size == 0, threshold > 0 and finite; and the
 *     sizes the 32-bit indices of the kernels allow: group_size <= (2^31 - 1) / 4, n_points <= 2^40, groups * hypotheses <=
 *     2^25, 0 <= group_offset <= 2^31; min_conf, baseline, distance_thresh not NaN: else SKIMI_ERR_ARG before any launch.  Results are bitwise reproducible, and a group is bitwise what it is alone with the
 *     matching group_offset.
 * ws: at least skimi_essential_workspace_bytes(...) bytes (0 for sizes that skimi_essential_ransac refuses). */
size_t skimi_essential_workspace_bytes(int64_t n_points, int64_t group_size, int32_t hypotheses);
int skimi_essential_ransac(const double* x2d, const double* conf, const double* K, int64_t n_points, int64_t group_size,
                           double min_conf, double threshold, int32_t hypotheses, uint64_t seed, int64_t group_offset,
                           double baseline, double distance_thresh, double* R, double* t, double* E, uint8_t* inliers,
                           uint8_t* pose_mask, int32_t* n_used, int32_t* n_inliers, int32_t* n_pose, int32_t* cheirality,
                           double* cost, int32_t* winner, int32_t* n_solutions, double* confidence, int32_t* success,
                           void* ws, size_t ws_bytes, void* stream);
/* Rule 4 alone, one thread per sample: a, b dev f64 [samples, 5, 2] normalised coordinates -> E [samples, 10, 3, 3] (the
 * first counts[s] are solutions, the rest NaN), counts [samples] i32. */
int skimi_five_point(const double* a, const double* b, int64_t samples, double* E, int32_t* counts, void* stream);

/* The filtered, coloured point cloud of a time step (predictions_to_glb, vggt/visual_util.py:39-236, which runs in NumPy
 * on the host).  A scene is one step: n = S H W pixels in view-major, row-major order; all B scenes go through every launch.
 * Inputs (dev f32): points [B, S, H, W, 3]; conf [B, S, H, W]; images [B, S, 3, H, W] (images_nchw != 0) or
 * [B, S, H, W, 3]; extrinsic [B, S, 3, 4].  Rules (DESIGN §2 "Scene cloud", restated in tests/scene_restated.py):
 *  1. colour = (uint8)(float32(v) * 255.0f), truncated toward zero; NaN -> 0, below 0 -> 0, >= 256 -> 255.
 *  2. thr: conf_thres == 0 -> 0; else the conf_thres-th percentile of the scene's conf by NumPy's `linear` method in float64
 *     on the exact order statistics: v = q / 100 (n - 1), i = floor(v), g = v - i, lo = s[i], hi = s[min(i + 1, n - 1)],
 *     d = hi - lo, thr = lo + d g if g < 0.5 else hi - d (1 - g).  The order is that of the order-preserving 32-bit key
 *     (-0.0 just below +0.0, +-inf ordered).  Any NaN conf: thr = lo = hi = NaN and nothing is kept (thr stays 0 at
 *     conf_thres == 0, where a NaN conf is merely not kept).
 *  3. kept: (double)conf >= thr and conf > float32(1e-5); mask_black_bg: R + G + B >= 16; mask_white_bg: not (R, G, B all
 *     > 240).  Non-finite points are not filtered; their number among the kept is reported.
 *  4. the kept pixels go to xyz [B, cap, 3] f32 and rgb [B, cap, 3] u8 in pixel order; count [B] i64 is the full number
 *     kept; beyond row min(count, cap) - 1 nothing is written.
 *  5. per axis the 5th and 95th percentile (rule 2's lerp) of ALL kept raw vertices -> lower, upper; scale = ||upper -
 *     lower|| in float64.  A kept NaN in an axis: that axis's percentiles and the scale are NaN.  count == 0: lower = upper =
 *     NaN, scale = 1.
 *  6. transform [B, 4, 4] f64 = E0^-1 diag(-1, -1, 1, 1), E0 the 4 x 4 of view 0, its 3 x 3 inverted by the adjugate in
 *     float64 (a general inverse).  align != 0: the written xyz is float32(A (x, y, z, 1)) formed in float64; else raw.
 *  7. stats [B, 16] f64 = thr, lo, hi, NaN confs, non-finite kept vertices, lower[3], upper[3], scale, count, 0, 0, 0.
 * 1 <= n <= (2^31 - 1) / 3, 1 <= B <= 65535, 0 <= conf_thres <= 100, cap >= 1.  workspace: skimi_scene_workspace_bytes(B, n)
 * bytes (0 for sizes out of range).  skimi_scene_tile(n): the consecutive pixels one workgroup handles per pass;
 * ceil(n / tile) workgroups per scene.  Ten launches whatever the data, no synchronisation, no allocation, no
 * floating-point atomics (integer histograms and counters only): results are bitwise reproducible, and a scene's results
 * are bitwise the same alone or inside a batch.  Bad arguments: SKIMI_ERR_ARG before any launch. */
int64_t skimi_scene_tile(int64_t n);
size_t skimi_scene_workspace_bytes(int64_t B, int64_t n);
int skimi_scene_cloud(const float* points, const float* conf, const float* images, const float* extrinsic, int64_t B, int32_t S,
                      int32_t H, int32_t W, int32_t images_nchw, double conf_thres, int32_t mask_black_bg, int32_t mask_white_bg,
                      int32_t align, int64_t cap, void* workspace, float* xyz, uint8_t* rgb, int64_t* count, double* stats,
                      double* transform, void* stream);

/* Fusion and temporal smoothing of a clip's joints on the device (the host functions of fuse.py are the restatement:
 * VideoPose3D/fuse/fuse.py + fuse_check.py, fuse/main_raw.py:194-250, fuse/fuse.py:289-412, fuse/confidence.py,
 * triangulation/postprocess.py:54-67).  All arithmetic float64, compiled without FMA contraction; inputs and outputs are dev
 * f64 except status / fit_ok (dev i32).  One launch per call, no synchronisation, no allocation, no atomics; every sum is a
 * lane's own sum over its joints followed by a fixed butterfly over the wave, so results are bitwise reproducible, a frame's
 * results do not depend on `frames` or on the frame's position, and a joint's smoothed series does not depend on the other
 * joints.  frames == 0 is valid and launches nothing.  Bad arguments: SKIMI_ERR_ARG before any launch, outputs untouched.
 * Rules (DESIGN §2 "Fusion + smoothing on the device"):
 *
 * skimi_fuse_h36m = fuse_pose_no_extrinsics_h36m per frame.  left, right [frames, 17, 3]; tau_j [17] or NULL (then the
 * scalar tau); wL, wR NULL (all ones) or [17] (stride 0) or [frames, 17] (stride 17).
 *  1. mirror_right_x: the right view's x and z negated.  center_scale_h36m of both views: pelvis (joint 0) to the origin,
 *     divided by the pelvis-neck (joint 9) distance d unless d > 1e-8 is false (then by 1).
 *  2. estimate_rigid_umeyama on the torso joints 0, 9, 4, 1, 11, 14 finite on both sides (n of them; n < 3: rule 6): Sigma =
 *     Yc^T Xc / n (X left, Y right, centred) = U S V^T; R = U V^T (the reference's quirk: the transpose of the least-squares
 *     rotation), with the last column of U flipped when det R < 0; s = sum S / (||Yc||^2 / n + 1e-12) if allow_scale else 1;
 *     t = mean X - s R mean Y.  The SVD is a one-sided Jacobi to convergence; R is formed from the two largest singular
 *     triplets and their cross products, which equals the rule for every sign choice of an SVD (rank(Sigma) < 2 is open).
 *  3. fuse_two of the left pose and s R right + t per joint: the only finite side; both finite: ||L - R|| > tau_j picks the
 *     side of the larger weight (left on a tie), else (wL L + wR R) / (wL + wR + 1e-9); neither: NaN.
 *  4. center_scale_h36m of the result -> fused [frames, 17, 3].
 *  5. diag [frames, 4] = LR_before, Fused_vs_L, Fused_vs_R, gain: the plain means over the 17 joints of ||Ln - Rn||, ||fused -
 *     Ln||, ||fused - Rn|| (NaN-propagating) and LR_before - (Fused_vs_L + Fused_vs_R) / 2.  R [frames, 3, 3], t [frames, 3],
 *     s [frames], status [frames] = 1.
 *  6. n < 3, where the host raises ValueError: the frame's fused, R, t, s and diag are NaN and status = 0. */
int skimi_fuse_h36m(const double* left, const double* right, int64_t frames, double tau, const double* tau_j, const double* wL,
                    int64_t wL_stride, const double* wR, int64_t wR_stride, int32_t allow_scale, int32_t mirror_right_x,
                    double* fused, double* R, double* t, double* s, double* diag, int32_t* status, void* stream);

/* skimi_fuse_views = the per-frame body of fuse/main_raw.py:194-240.  X_l, X_r [frames, joints, 3]; U_l, U_r [frames, joints,
 * 2] pixels; 1 <= joints <= 128; the five key joints in 0 .. joints - 1; sigma_px, sigma_3d finite; min_points >= 1.
 *  1. align_right_to_left: on the joints finite in both views (fewer than 3: aligned = X_r), Kabsch R = V U^T of (X_r -
 *     mean)^T (X_l - mean) = U S V^T with the last column of V flipped when det R < 0 (SVD as in skimi_fuse_h36m), t = mean_l
 *     - R mean_r; aligned = R X_r + t on those joints, X_r elsewhere.
 *  2. weakpersp_reproj_confidence of each view on its RAW 3D: on the rows finite in X and U, M = P[:, :2] Q^T of Xc^T Uc = P S
 *     Q^T, s = sum S / sum Xc^2, t = mean U - s mean X M; err = ||s X M + t - U|| where both are finite, else NaN; conf =
 *     exp(-err^2 / (2 max(sigma_px, 1e-12)^2)), 0 where err is NaN.  Fewer than min_points rows, or sum Xc^2 < 1e-12, where
 *     the host raises: that view's conf is 0 and its err NaN for every joint of the frame, and its fit_ok = 0.
 *  3. crossview_consistency_confidence of the raw pair: canonicalize_pose_3d of each view (origin at the root, x = left hip ->
 *     right hip, y = hip centre -> shoulder centre made orthogonal to x, z = x cross y, unit vectors with eps 1e-9; divided
 *     by the hip width, SKIMI_FUSE_SCALE_HIP, or the hip-shoulder distance, SKIMI_FUSE_SCALE_TORSO; a non-finite key joint
 *     or a scale < 1e-9: all NaN); dist = the distance of the two canonical poses per joint, NaN where either is; conf_x =
 *     exp(-dist^2 / (2 max(sigma_3d, 1e-12)^2)), 0 where dist is NaN.
 *  4. q = sqrt(conf conf_x) per view; fuse_frame_3d(X_l, aligned, q_l, q_r): softmax2 weights w = exp(q - max) / (sum + 1e-8);
 *     a joint present on one side takes that side, on both (wl X_l + wr aligned) / (wl + wr + 1e-8), on neither NaN.
 * Outputs: fused, aligned [frames, joints, 3]; q_l, q_r, conf_l, conf_r, conf_x, err_l, err_r, dist [frames, joints]; fit_ok
 * [frames, 2] i32 (left, right). */
#define SKIMI_FUSE_SCALE_HIP 0
#define SKIMI_FUSE_SCALE_TORSO 1
int skimi_fuse_views(const double* X_l, const double* X_r, const double* U_l, const double* U_r, int64_t frames, int32_t joints,
                     int32_t root_idx, int32_t left_hip_idx, int32_t right_hip_idx, int32_t left_shoulder_idx,
                     int32_t right_shoulder_idx, double sigma_px, double sigma_3d, int32_t scale_mode, int32_t min_points,
                     double* fused, double* aligned, double* q_l, double* q_r, double* conf_l, double* conf_r, double* conf_x,
                     double* err_l, double* err_r, double* dist, int32_t* fit_ok, void* stream);

/* skimi_smooth_ema = temporal_smooth_ema.  X, Y [frames, joints, 3] (Y must not be X); base [joints]: the per-joint base
 * factor clip(alpha factor, alpha_min, alpha_max) when adaptive, alpha itself otherwise.  One thread per joint, sequential
 * in t.  Y[0] = X[0] bit for bit; then per step a joint is (three finite coordinates now) + 2 (the previous OUTPUT row is
 * finite): 0 -> NaN, 1 -> the observation, 2 -> the previous output, 3 -> a x + (1 - a) y with a = min(max(base + speed_gain
 * ||x - y||, alpha_min), alpha_max) (adaptive) or base; two products and a sum, no fused multiply-add. */
int skimi_smooth_ema(const double* X, int64_t frames, int64_t joints, const double* base, int32_t adaptive, double alpha_min,
                     double alpha_max, double speed_gain, double* Y, void* stream);

/* skimi_smooth_ema_batch = skimi_smooth_ema on `clips` clips at once: X, Y [clips, frames, joints, 3], one base [joints] for
 * all of them.  One launch, one thread per (clip, joint) running skimi_smooth_ema's walk: clip b's result is that call's on
 * X[b] bit for bit.  clips == 0 is valid and launches nothing. */
int skimi_smooth_ema_batch(const double* X, int64_t clips, int64_t frames, int64_t joints, const double* base, int32_t adaptive,
                           double alpha_min, double alpha_max, double speed_gain, double* Y, void* stream);

/* skimi_fuse_group = fuse/main_unity.py:98-132 (align == 0) or the per-frame body of fuse/main_raw.py:194-240 (align != 0) for
 * every pair (a, b), a < b, of `views` views, pairs in the order of itertools.combinations: pair p of P = views (views - 1)
 * / 2.  X [views, frames, joints, 3]; U [views, frames, joints, 2].  Rules (DESIGN §2 "Group fusion"): those of
 * skimi_fuse_views with X_l = X[a], X_r = X[b], through the same device code:
 *  1. quality == NULL: rule 2 (conf, err [views, frames, joints], fit_ok [views, frames]) and the canonical pose of rule 3
 *     (workspace, skimi_fuse_group_workspace_bytes) once per (view, frame) in a first launch; then per (pair, frame) rule 1
 *     if align, else aligned = X[b]; dist and conf_x of rule 3; q_a = sqrt(conf[a] conf_x), q_b = sqrt(conf[b] conf_x);
 *     rule 4.  (main_unity's clip(conf conf_x, 0, 1) changes nothing: both factors lie in [0, 1].)  With align != 0 every
 *     output of pair (a, b) equals skimi_fuse_views' on (X[a], X[b], U[a], U[b]) bit for bit.
 *  2. quality [views, frames, joints] given: q_a = quality[a], q_b = quality[b]; one launch; U, workspace, conf, err,
 *     fit_ok, conf_x and dist are not touched and may be NULL.
 * Outputs per pair: fused, aligned [P, frames, joints, 3]; q_a, q_b, conf_x, dist [P, frames, joints].  views <= 4096, views *
 * frames and P * frames below 2^31.  views < 2 gives no pair (views == 1 still fills conf, err, fit_ok).  A pair's results
 * depend on its two views alone. */
size_t skimi_fuse_group_workspace_bytes(int64_t views, int64_t frames, int32_t joints);
int skimi_fuse_group(const double* X, const double* U, const double* quality, int64_t views, int64_t frames, int32_t joints,
                     int32_t root_idx, int32_t left_hip_idx, int32_t right_hip_idx, int32_t left_shoulder_idx,
                     int32_t right_shoulder_idx, double sigma_px, double sigma_3d, int32_t scale_mode, int32_t min_points,
                     int32_t align, void* workspace, size_t workspace_bytes, double* fused, double* aligned, double* q_a, double* q_b,
                     double* conf_x, double* dist, double* conf, double* err, int32_t* fit_ok, void* stream);

/* skimi_joint_quality = the ground-truth-free joint quality of fuse/fuse.py:124-285 (estimate_bone_median_lengths,
 * q_from_bone_deviation, q_from_temporal, q_2d_sanity, combine_q) for `views` clips.  X [views, frames, joints, 3] (NaN rows =
 * missing joints); U [views, frames, joints, 2] or NULL; edges [n_edges, 2] dev i32, positions on the joint axis; size [views,
 * 2] dev f64 (width, height), needed with U; bias NULL, [joints] (bias_stride 0) or [views, joints] (bias_stride joints);
 * med_lens [views, n_edges]: written, or read when med_given.  Two launches (one when med_given or n_edges == 0), no
 * atomics, bitwise reproducible; a view's results depend on that view alone, and with med_given a frame's on that frame
 * and the one before it.  Rules (DESIGN §2 "Joint quality"):
 *  - a row is finite when its three coordinates are.  len[v, t, e] = ||X[a] - X[b]|| when both rows are finite, else NaN.
 *    An edge with an endpoint outside 0 .. joints - 1 is ignored everywhere (its median is NaN); edges act in their order,
 *    a repeated edge counts twice, a self-edge is counted twice for its joint.
 *  - med[v, e]: the median of the non-NaN len[v, :, e], an exact selection on order-preserving keys (one wave per (view,
 *    edge)); (lo + hi) / 2 for an even count; NaN without a sample (frames == 0 included).
 *  - q_bone: -1e9 for a row that is not finite; else over the edges at j with a finite median and two finite rows, dev_sum
 *    += |len - med| in edge order and cnt of them: -100 for cnt == 0, else -(dev_sum / (cnt + 1e-8)).
 *  - q_temp: -1e9 for a row that is not finite; 0 for t == 0 or a row at t - 1 that is not finite; else -beta_temp ||X[t] -
 *    X[t-1]||.
 *  - q_san: 0 where U is given, u and v are finite and 0 <= u < width, 0 <= v < height; else -50.
 *  - q = (w_bone q_bone + w_temp q_temp) + w_san q_san, then + bias if given, in this order, no fused multiply-add.
 * q, q_bone, q_temp, q_san [views, frames, joints].  1 <= joints <= 128, views <= 4096, n_edges <= 65536, views * frames
 * below 2^31. */
int skimi_joint_quality(const double* X, const double* U, int64_t views, int64_t frames, int32_t joints, const int32_t* edges,
                        int32_t n_edges, const double* size, double beta_temp, double w_bone, double w_temp, double w_san,
                        int32_t med_given, const double* bias, int64_t bias_stride, double* med_lens, double* q, double* q_bone,
                        double* q_temp, double* q_san, void* stream);

/* skimi_convert_skeleton = VideoPose3D/coco_hm36.py (coco_to_h36m, h36m_to_coco) on the device.  X, Y [frames, 17, coords],
 * coords 2 or 3 (Y must not be X); one launch, one thread per frame; NaN propagates through the arithmetic.  frames <= 2^34,
 * but <= 2^20 for SKIMI_SKELETON_H36M_TO_COCO with synthesize: every workgroup of 256 frames sums the clip mean below
 * itself, frames^2 / 256 reads in all, the price of one launch and of the same bits in every frame.  Rules (DESIGN
 * §2 "Skeleton conversion"):
 *  - SKIMI_SKELETON_COCO_TO_H36M: pelvis = (l_hip + r_hip) 0.5, thorax = (l_sho + r_sho) 0.5, spine = (pelvis + thorax) 0.5,
 *    neck = nose, head = nose + 0.5 (nose - (l_eye + r_eye) 0.5) if synthesize else nose; the 12 limb joints are copied.
 *  - SKIMI_SKELETON_H36M_TO_COCO: nose = neck, the 12 limb joints are copied, eyes and ears NaN unless synthesize.  With
 *    synthesize: sv = l_sho - r_sho, but the first `coords` entries of (1, 0, 0) in EVERY frame when the clip mean of ||sv||
 *    (summed in a fixed order; a NaN mean does not count) is < 1e-8, the reference's quirk; w = ||sv||, side = sv / (w +
 *    1e-9), up = (head - neck) / (||head - neck|| + 1e-9); l_eye, r_eye = (head +- 0.25 w side) - 0.15 w up; l_ear, r_ear =
 *    (head +- 0.35 w side) - 0.10 w up. */
#define SKIMI_SKELETON_COCO_TO_H36M 0
#define SKIMI_SKELETON_H36M_TO_COCO 1
int skimi_convert_skeleton(const double* X, int64_t frames, int32_t coords, int32_t direction, int32_t synthesize, double* Y,
                           void* stream);

/* skimi_smooth_savgol = smooth_skeleton with the window already chosen.  X, Y [frames, joints, 3] (Y must not be X); win odd
 * in 1..33, 0 <= poly < win (poly is only checked); fir [win]; first, last [win / 2, win] (fuse.savgol_operators).  One thread
 * per (joint, coordinate) series: its finite samples in time order form the sequence x_0 .. x_{n-1}; with n >= win, y_k =
 * sum_m fir[m] x_{k - win/2 + m} for win/2 <= k < n - win/2, y_e = sum_m first[e][m] x_m and y_{n - win/2 + e} = sum_m
 * last[e][m] x_{n - win + m} for e < win/2 (sums in ascending m), written back to the samples' own time steps.  Non-finite
 * samples, and series with n < win, pass through bit for bit. */
int skimi_smooth_savgol(const double* X, int64_t frames, int64_t joints, int32_t win, int32_t poly, const double* fir,
                        const double* first, const double* last, double* Y, void* stream);

/* Kinematic analysis of clips of 3D joints on the device: the 14 per-frame series of angle/main.py, their 28 change series,
 * the skier's facing heading, the split of each clip into turns and the per-turn statistics of all 42 series
 * (angle/main.py: compute_angles, compute_tilt_angles, compute_torso_knee_angle, compute_knee_difference,
 * compute_elbow_distance_from_midline, compute_facing_heading, compute_series_changes, detect_turn_segments and the
 * statistics of save_turn_reports; tests/kinematics_restated.py is the restatement).  All arithmetic float64, compiled
 * without FMA contraction.  Three launches for all clips (two when frames == 0, none when clips == 0), no synchronisation,
 * no allocation, no floating-point atomics; the turn count stays on the device.  Every sum runs in an order that depends
 * only on positions inside the clip (or inside the turn), so results are bitwise reproducible and a clip's results are the
 * same bits alone or in a batch, at any place in it, in either placement (below), whatever lies beyond its length.
 * Bad arguments: SKIMI_ERR_ARG before any launch, outputs untouched.  Rules (DESIGN §2 "Kinematics"):
 *
 * Input.  X [clips, frames, joints, 3] dev f64; lengths [clips] dev i32 or NULL (every clip has `frames` frames).  A length
 * is clamped to 0 .. frames on the device.  Frames at or beyond a clip's length are never read: there the series, heading,
 * heading_smooth and velocity_smooth are NaN and boundary is 0, and everything below speaks of the clip's first `length`
 * frames, T of them.  layout [13] (host): the joint index of each role, SKIMI_KIN_SHOULDER_L .. SKIMI_KIN_NECK, in 0 ..
 * joints - 1, or -1 for absent; an absent role behaves as a non-finite joint.  up [3] (host), finite and not zero.
 *
 * The 14 base series, series[:, 0..13, :] of series [clips, 42, frames]:
 *  0-7  knee_l, knee_r, elbow_l, elbow_r, shoulder_l, shoulder_r, hip_l, hip_r: the angle ABC in degrees of (hip, knee,
 *       foot), (shoulder, elbow, hand), (neck, shoulder, elbow), (neck, hip, knee): NaN unless the three joints are finite
 *       and |BA| and |BC| are non-zero; acos of BA.BC / (|BA| |BC|) clipped to [-1, 1], times 180 / pi.
 *  8    torso_knee_angle: the angle (shoulder centre, pelvis centre, knee centre).  A centre is the mean of the finite ones
 *       of its two joints (hips, shoulders, knees): (a + b) / 2, the one finite joint, or NaN.
 *  9    knee_diff_lr = knee_l - knee_r where both are finite.
 *  10-11 elbow_distance_l, _r = sqrt(dx^2 + dz^2) of the elbow from the pelvis centre, both finite.
 *  12-13 tilt_upper, tilt_lower of v = shoulder centre - pelvis centre and knee centre - pelvis centre: lr = hip_r - hip_l when
 *       both hips are finite, else shoulder_r - shoulder_l when both are, else the frame has no tilt and no heading; l =
 *       lr / |lr|, u = up / |up|, forward f = unit(u x l) when up[1] < 0, else unit(l x u) (a zero or non-finite norm
 *       anywhere: no tilt, no heading).  p = unit(v - (v.l) l); tilt = acos(clip(p.u)) 180 / pi, negated where p.f >= 0 is
 *       false.  heading [clips, frames] = atan2(f.x, f.z) 180 / pi.
 * The 28 change series, series[:, 14 + 2k] = name_d and series[:, 15 + 2k] = name_abs_d of base series k: d[i] = s[i] - s[i-1]
 * where both are finite, else NaN, NaN at i = 0; abs_d = |d|.
 *
 * Turns of a clip (detect_turn_segments):
 *  1. Fewer than 5 finite headings: no turns, heading_smooth and velocity_smooth NaN.
 *  2. Fill: a non-finite heading at i between the nearest finite ones at l < i < r is (h[r] - h[l]) / (r - l) * (i - l) + h[l];
 *     before the first / after the last finite one it is that one's value (np.interp).
 *  3. Unwrap (np.unwrap, period 2 pi) of p = h pi / 180: dd = p[i] - p[i-1]; m = mod(dd + pi, 2 pi) - pi with the sign of the
 *     divisor, m = pi where m == -pi and dd > 0; correction c = m - dd, 0 where |dd| < pi; p[i] += c[1] + .. + c[i]; back to
 *     degrees with 180 / pi.  The running sum is a fixed blocked prefix sum: chunks of ceil(T / 256) samples in time order,
 *     then the chunk totals in order.
 *  4. heading_smooth [clips, frames] = box mean of window heading_window: the sum over the samples of i - w/2 .. i + w/2 that
 *     lie inside the clip, in ascending order, divided by their number.  This is also the rule for T < window, where the
 *     reference raises IndexError (np.convolve(mode="same") then returns the window's length); for T >= window the two agree.
 *  5. velocity = np.gradient: (s[i+1] - s[i-1]) / 2 inside, s[1] - s[0] and s[T-1] - s[T-2] at the ends;
 *     velocity_smooth [clips, frames] = its box mean of window velocity_window.
 *  6. Extrema: the i >= 1 with v[i-1] v[i] < 0.  Boundaries: 0; then, greedily, the first extremum >= min_turn_frames after
 *     the last boundary; then T - 1 (unless it already is the last boundary).
 *  7. A segment (s, e) of consecutive boundaries is a turn unless e - s + 1 < min_turn_frames or |hs[e] - hs[s]| <
 *     min_heading_change_deg.  Kept turns are numbered from 0 in time order: turn_frames [clips, max_turns, 2] i32 = (s, e),
 *     turn_heading_change [clips, max_turns] = hs[e] - hs[s], turn_direction [clips, max_turns] i32 = +1 where that is > 0,
 *     else -1; n_turns [clips] i32; boundary [clips, frames] u8 = 1 at the s and e of kept turns.  max_turns must be
 *     (frames - 1) / min_turn_frames + 1 (0 for frames == 0): boundaries after 0 are >= min_turn_frames apart, so at most
 *     (T - 1) / min_turn_frames extrema are taken and T - 1 adds at most one segment.
 *  8. turn_stats [clips, max_turns, 42, 4] = mean, population std, min, max of each series over the finite samples of [s, e],
 *     turn_counts [clips, max_turns, 42] i32 their number; no finite sample: four NaN.  One wave per (clip, turn, series): each
 *     lane sums samples s + lane, s + lane + 64, .. in time order, then a fixed xor butterfly; the std is a second pass over
 *     the deviations from that mean.
 *  9. Rows at and beyond n_turns: turn_frames, turn_direction and turn_counts 0; turn_heading_change and turn_stats NaN.
 *
 * Placement.  The per-clip arrays of rules 2-6 (three of `frames` doubles) live in LDS when workspace is NULL, which needs
 * frames <= SKIMI_KIN_LDS_FRAMES, and otherwise in workspace (dev), at least skimi_kin_workspace_bytes(clips, frames) bytes
 * (0 for negative sizes).  Both placements run the same code on the same values. */
#define SKIMI_KIN_SERIES 42
#define SKIMI_KIN_BASE_SERIES 14
#define SKIMI_KIN_ROLES 13
#define SKIMI_KIN_LDS_FRAMES 2048
enum {
    SKIMI_KIN_SHOULDER_L = 0, SKIMI_KIN_SHOULDER_R, SKIMI_KIN_ELBOW_L, SKIMI_KIN_ELBOW_R, SKIMI_KIN_HIP_L, SKIMI_KIN_HIP_R,
    SKIMI_KIN_KNEE_L, SKIMI_KIN_KNEE_R, SKIMI_KIN_FOOT_L, SKIMI_KIN_FOOT_R, SKIMI_KIN_HAND_L, SKIMI_KIN_HAND_R, SKIMI_KIN_NECK
};
size_t skimi_kin_workspace_bytes(int64_t clips, int64_t frames);
int skimi_kinematics(const double* X, const int32_t* lengths, int64_t clips, int64_t frames, int32_t joints,
                     const int32_t* layout, const double* up, int32_t min_turn_frames, double min_heading_change_deg,
                     int32_t heading_window, int32_t velocity_window, int32_t max_turns, void* workspace,
                     size_t workspace_bytes, double* series, double* heading, double* heading_smooth, double* velocity_smooth,
                     uint8_t* boundary, int32_t* n_turns, int32_t* turn_frames, double* turn_heading_change,
                     int32_t* turn_direction, double* turn_stats, int32_t* turn_counts, void* stream);

/* ---- pose evaluation: the MPJPE protocols and the ground-truth-free quality of clips (csrc/evaluate.hip) ----
 * Everything is float64 on the device, nothing is read back, no floating-point atomics: results are bitwise reproducible,
 * and a clip's results are the same bits alone or anywhere in a ragged batch.  lengths: NULL or [clips] i32 (dev), clamped
 * to 0 .. frames; the frames at and beyond a clip's length are never read.  Sizes: 0 <= clips < 2^31, 0 <= frames < 2^31 -
 * 64, 1 <= joints <= SKIMI_EVAL_MAX_JOINTS, clips * frames < 2^31, clips * joints < 2^31, clips * frames * joints * 3 <=
 * 2^40; clips == 0 launches nothing.  Bad arguments: SKIMI_ERR_ARG before any launch, outputs untouched.
 * Rules (DESIGN §2 "Evaluation"; T = frames, J = joints, n = the clip's length):
 *
 * skimi_pose_errors = VideoPose3D/common/loss.py (mpjpe, p_mpjpe, n_mpjpe, mean_velocity_error) with the per-joint tables of
 * metrics/unity_data_compare.py (calculate_per_joint_errors, summarize_joint_errors) and the mask of fuse_eval.
 * mean_pairwise_distance, for a batch of (pred, target) clips [clips, T, J, 3] in three launches (two when frames == 0).
 *  1. zero_root: a joint index or -1.  With zero_root >= 0 that joint of the target counts as (0, 0, 0) (VideoPose3D/run.py:994)
 *     and the stored values are not read.  A joint is valid in a frame when its six coordinates are finite; a frame is complete
 *     when all J joints are valid.  n_valid_f [clips, T] i32 = the frame's number of valid joints.
 *  2. err [clips, T, J] = ||p - g|| on valid joints, NaN elsewhere.  mpjpe_f [clips, T] = the mean of the frame's finite err,
 *     NaN without one.
 *  3. n_mpjpe_f [clips, T], complete frames only: scale = mean_j(g . p) / mean_j(p . p), the mean of ||scale p - g||; an
 *     incomplete frame or a non-finite result is NaN.
 *  4. Procrustes (loss.py:27-66), complete frames only: X0 = g - mean(g), Y0 = p - mean(p), each divided by its Frobenius norm,
 *     H = X0^T Y0 = U S V^T, R = V U^T with the last column of V and the last singular value negated when det R < 0 (here:
 *     the polar factor of svd3.h, which is that whatever signs an SVD chose), a = sum(S) ||X0|| / ||Y0||, t = mean(g) - a
 *     mean(p) R, aligned = a p R + t.  p_err [clips, T, J] = ||aligned - g||, p_mpjpe_f [clips, T] its mean; aligned
 *     [clips, T, J, 3], p_R [clips, T, 3, 3], p_scale [clips, T], p_t [clips, T, 3] are optional (NULL: not written).
 *     p_status [clips, T] i32 = 1 where the frame is complete, both poses have extent (norms > 0) and every result is
 *     finite; else 0 and all Procrustes outputs of the frame are NaN (the reference raises or returns NaN there).
 *  5. vel_err [clips, T, J], t >= 1: ||(p_t - p_{t-1}) - (g_t - g_{t-1})|| where the joint is valid in both frames, else NaN;
 *     row 0 is NaN.
 *  6. Rows at and beyond n: every per-frame float NaN, n_valid_f and p_status 0.
 *  7. metrics [clips, 4] (SKIMI_PE_*): MPJPE = the mean of the clip's finite err; P_MPJPE, N_MPJPE = the mean of the per-frame
 *     value over the frames that have a finite one; MPJVE = the mean of the finite vel_err.  An empty mean is NaN.  counts
 *     [clips, 3] i32 = n_err, n_complete, n_vel.  One workgroup per clip: thread i sums the samples i, i + 256, .. of the
 *     clip's n J (or n) samples, then a fixed xor butterfly per wave, then the four wave totals in order.
 *  8. joint_stats [clips, 2, J, 3] = mean, population std (two passes: the mean, then the deviations), median of a joint's
 *     finite err (table 0) and p_err (table 1) over the clip; joint_n [clips, 2, J] i32 their number, 0: three NaN.  The
 *     median is the mean of the two middle order statistics (one for an odd count), selected exactly.
 *
 * skimi_clip_quality = the figures of VideoPose3D/fuse/fuse_eval.py (bone_lengths, eval_fused_pose's CV and symmetry,
 * temporal_stats, symmetry_score_mirror) and metrics/true_data_compare.py (compute_temporal_metrics, compute_bone_length_cv)
 * for a batch of clips X [clips, T, J, 3] in one launch.  edges [n_edges, 2], left_edges, right_edges, lr_pairs [n_pairs, 2]
 * as (left, right): i32 joint indices on the HOST, at most SKIMI_EVAL_MAX_EDGES edges per list and SKIMI_EVAL_MAX_PAIRS pairs.
 *  1. L[t, e] = the distance of the edge's joints, NaN unless both are finite.  bone_len [clips, T, n_edges] (optional): L,
 *     NaN at and beyond n.
 *  2. scalars [clips, SKIMI_CQ_SCALARS]:
 *     BONE_CV_POOLED = nanstd(L) / (nanmean(L) + 1e-9) over all (t, e); no length: NaN.
 *     BONE_CV_MEAN = the mean of bone_cv_edge over the edges that have a value, in edge order; none: NaN.  bone_cv_edge
 *       [clips, n_edges] = std / mean of the edge's lengths where it has one and the mean exceeds 1e-9, else NaN.
 *     LR_LENGTH_SYMMETRY = |Lm - Rm| / (0.5 (Lm + Rm) + 1e-9), Lm, Rm the nanmeans over left_edges and right_edges.
 *     SPEED_MEAN, JERK_MEAN = the mean norm of the first / second differences, over the (frame, joint) where all three
 *       coordinates of the difference are finite; n < 3 or no such sample: NaN.
 *     SPEED_P95, ACCEL_P95: every (joint, coordinate) series with at least 2 finite samples is filled as np.interp over the
 *       frame index does (linear inside, the end values held outside), the others stay as they are; then NumPy's `linear`
 *       95th percentile of the (n - 1) J norms of the first and of the (n - 2) J norms of the second differences, by exact
 *       selection.  A NaN among the values: NaN.  n < 3: NaN.
 *     MIRROR_SYMMETRY = over the pairs finite on both sides in frame n - 1, in pair order, the mean of ||X[l] - (-x, y, z)
 *       of X[r]||; n == 0 or no pair: NaN.
 *  3. Placement.  The filled clip and the two series of norms (five of frames * joints doubles) live in LDS when workspace is
 *     NULL, which needs frames * joints <= SKIMI_EVAL_LDS_ELEMS, and otherwise in workspace (dev), at least
 *     skimi_eval_workspace_bytes bytes (0 for sizes the call refuses).  Both placements run the same code on the same values. */
#define SKIMI_EVAL_MAX_JOINTS 128
#define SKIMI_EVAL_MAX_EDGES 128
#define SKIMI_EVAL_MAX_PAIRS 64
#define SKIMI_EVAL_LDS_ELEMS 1440
enum { SKIMI_PE_MPJPE = 0, SKIMI_PE_P_MPJPE, SKIMI_PE_N_MPJPE, SKIMI_PE_MPJVE };
enum {
    SKIMI_CQ_BONE_CV_POOLED = 0, SKIMI_CQ_BONE_CV_MEAN, SKIMI_CQ_LR_LENGTH_SYMMETRY, SKIMI_CQ_SPEED_MEAN, SKIMI_CQ_JERK_MEAN,
    SKIMI_CQ_SPEED_P95, SKIMI_CQ_ACCEL_P95, SKIMI_CQ_MIRROR_SYMMETRY, SKIMI_CQ_SCALARS
};
size_t skimi_eval_workspace_bytes(int64_t clips, int64_t frames, int32_t joints);
int skimi_pose_errors(const double* pred, const double* target, const int32_t* lengths, int64_t clips, int64_t frames, int32_t joints,
                      int32_t zero_root, double* err, double* p_err, double* vel_err, double* mpjpe_f, double* n_mpjpe_f,
                      double* p_mpjpe_f, int32_t* n_valid_f, int32_t* p_status, double* aligned, double* p_R, double* p_scale,
                      double* p_t, double* metrics, int32_t* counts, double* joint_stats, int32_t* joint_n, void* stream);
int skimi_clip_quality(const double* X, const int32_t* lengths, int64_t clips, int64_t frames, int32_t joints, const int32_t* edges,
                       int32_t n_edges, const int32_t* left_edges, int32_t n_left, const int32_t* right_edges, int32_t n_right,
                       const int32_t* lr_pairs, int32_t n_pairs, void* workspace, size_t workspace_bytes, double* scalars,
                       double* bone_cv_edge, double* bone_len, void* stream);

/* ---- lens distortion: OpenCV's rational + tangential + thin-prism model on points and frames (csrc/lens.hip) ----
 * Everything is float64 on the device, one launch per call, bitwise reproducible (no data-dependent exit, no atomics).
 * Rules (DESIGN §2 "Lens distortion"; tests/lens_restated.py evaluates the same expressions in the same order):
 *  1. Parameters are HOST arrays, one set per camera, 1 <= C <= SKIMI_LENS_MAX_CAMERAS, and reach the kernel by value.
 *     K, P, new_K [C, 3, 3] are read as fx = [0][0], fy = [1][1], cx = [0][2], cy = [1][2]; the other entries are not part of
 *     the model.  dist [C, 12] = k1 k2 p1 p2 k3 k4 k5 k6 s1 s2 s3 s4 (shorter OpenCV vectors zero-padded by the caller; the
 *     tilt terms are not supported); NULL: all zero.  A zero or non-finite focal length, a non-finite principal point or
 *     coefficient: SKIMI_ERR_ARG.
 *  2. The model on normalised (x, y): r2 = x x + y y, c = (1 + k1 r2 + k2 r2^2 + k3 r2^3) / (1 + k4 r2 + k5 r2^2 + k6 r2^3),
 *     x_d = x c + 2 p1 x y + p2 (r2 + 2 x x) + s1 r2 + s2 r2^2, y_d = y c + p1 (r2 + 2 y y) + 2 p2 x y + s3 r2 + s4 r2^2.
 *  3. Points are [outer, C, n, 2] (dev): camera c owns the rows (o, c, .) of every o; outer = 1 is the plain [C, n, 2].
 *     outer * n <= 2^31; an empty call launches nothing.  K_steps (dev, or NULL) [outer, C, 3, 3]: the K of every
 *     (o, c), read from memory in place of the by-value K, with P = K (P must then be NULL and K may be).
 *  4. skimi_distort_points: undistorted points -> distorted pixels of K.  The input is pixels of P (NULL: K), or normalised
 *     coordinates when normalized != 0.
 *  5. skimi_undistort_points: distorted pixels of K -> undistorted points, as pixels of P (NULL: K) or, normalized != 0, as
 *     normalised coordinates.  OpenCV's fixed-point iteration from the distorted point: each of exactly `iters` rounds
 *     (0 .. SKIMI_LENS_MAX_ITERS; cv2.undistortPoints runs 5) subtracts the tangential and prism terms and multiplies by 1 / c.
 *     resid_px [outer, C, n] = the distance, in pixels of K, between the input and the re-distorted result: large where the
 *     iteration did not converge or the point lies outside the model's invertible range.  A non-finite result or residual
 *     (a NaN keypoint included) makes the point's two coordinates and its residual NaN; no other row is affected.
 *  6. skimi_project_points = cv2.projectPoints with rotation matrices: X [outer, C, n, 3] (dev), R [C, 3, 3], t [C, 3] (host)
 *     -> Xc = R X + t, (x, y) = (Xc_x, Xc_y) / Xc_z, rule 2, px [outer, C, n, 2] = pixels of K, depth [outer, C, n] = Xc_z.
 *     Points at or behind the camera are projected as the formula says (inf / NaN at Xc_z = 0), as cv2 does.
 *  7. skimi_undistort_u8 = cv2.undistort with a constant (0) border: in [C, F, H, W, ch] u8 -> out [C, F, OH, OW, ch] u8 (dev),
 *     ch 1, 3 or 4, sides 1 .. SKIMI_LENS_MAX_SIDE, C * F <= 65535.  Output pixel (u, v) -> x = (u - cx') / fx', y = (v - cy') /
 *     fy' through new_K (NULL: K) -> rule 2 -> (su, sv) = (fx x_d + cx, fy y_d + cy), computed on the fly (no stored map).
 *     Unless -1 < su < W and -1 < sv < H (a NaN fails) the pixel is 0.  Else x0 = floor(su), y0 = floor(sv), a = su - x0,
 *     b = sv - y0, taps outside the source count 0, value = (1 - b) ((1 - a) p00 + a p01) + b ((1 - a) p10 + a p11) in that
 *     order, out = floor(value + 0.5).  cv2.remap quantises (su, sv) to 1/32 px and uses integer weights: its grey levels
 *     may differ from these by a small amount; this rule is the contract.  The input is only read; nothing beyond the
 *     C F OH OW ch output bytes is written (dword stores when OW * ch % 4 == 0 and out is 4-byte aligned, else bytes). */
#define SKIMI_LENS_MAX_CAMERAS 8
#define SKIMI_LENS_MAX_ITERS 1000
#define SKIMI_LENS_MAX_SIDE 32768
int skimi_distort_points(const double* x, const double* K, const double* dist, const double* P, const double* K_steps,
                         int64_t outer, int32_t C, int64_t n, int32_t normalized, double* out, void* stream);
int skimi_undistort_points(const double* x, const double* K, const double* dist, const double* P, const double* K_steps,
                           int64_t outer, int32_t C, int64_t n, int32_t iters, int32_t normalized, double* out, double* resid_px,
                           void* stream);
int skimi_project_points(const double* X, const double* R, const double* t, const double* K, const double* dist, int64_t outer,
                         int32_t C, int64_t n, double* px, double* depth, void* stream);
int skimi_undistort_u8(const uint8_t* in, uint8_t* out, const double* K, const double* dist, const double* new_K, int32_t C,
                       int32_t F, int32_t H, int32_t W, int32_t OH, int32_t OW, int32_t ch, void* stream);

/* ---- bird's-eye view of the front camera: homography, frame warp, skeleton on the plan, ground track (csrc/bev.hip) ----
 * front_side/front/bev_utils.py (cv2.findHomography(method=0), image_points_to_bev, cv2.warpPerspective), front_side/run.py
 * (project_world_to_bev_centered + the centre of merge).  Everything is float64 on the device, one launch per call, no
 * atomics, no host synchronisation, no allocation, bitwise reproducible; a group's result is the same bits alone and inside
 * a batch.  Rules (DESIGN §2 "Bird's-eye view"; tests/bev_restated.py evaluates the same expressions in the same order):
 *
 * skimi_homography_fit: src, dst [G, n, 2] (dev), 4 <= n, G >= 1, G n <= 2^31; post [9] (HOST, NULL: identity, finite) ->
 * H, Hinv [G, 9], Hn [G, 9] (or NULL), err [G, n], stats [G, 4], status [G] i32 (dev).  One wave per group; every sum over the points is one lane's,
 * in point order.
 *  1. A correspondence is used iff its four numbers are finite; fewer than 4 used: the group fails.
 *  2. Hartley normalisation per side over the used points: centroid c, mean distance d, s = sqrt(2) / d, point -> (x - c) s.
 *     d = 0 or non-finite: the group fails.
 *  3. Each used pair (x, y) -> (u, v), normalised, gives the rows [-x, -y, -1, 0, 0, 0, u x, u y, u] and [0, 0, 0, -x, -y, -1,
 *     v x, v y, v]; the 9 x 9 A^T A is summed in point order.
 *  4. Cyclic Jacobi to convergence (csrc/jacobi.h: the stopping rule and zeroing of the essential matrix's null space); h =
 *     the eigenvector of the smallest eigenvalue, the lower index on a tie.
 *  5. Hn = T_dst^-1 h T_src.  |Hn[2][2]| >= 1e-12 ||Hn||_F: Hn /= Hn[2][2]; else Hn is scaled to ||Hn||_F = 1 with its entry
 *     of largest magnitude positive.
 *  6. status = 1 iff Hn is finite and |det Hn| >= 1e-12 (the reference's check_homography on H_m); else the group fails.
 *  7. H = post Hn, not renormalised (post = the canvas matrix S keeps h22 = 1: its last row is (0, 0, 1)).  The Hn output is
 *     rule 5's matrix itself (the reference's H_m beside its H_px = S H_m), NaN for a failed group.
 *  8. Hinv = adj(H) / det(H), every cofactor a b - c d in written order.
 *  9. A failed group: H, Hinv, err, rms and max all NaN, status 0; its neighbours are untouched.
 * 10. err = || pi(H x) - pi(post x') || per used point, NaN for an unused one; stats = n_used, rms err, max err, det Hn (NaN
 *     when the group failed before rule 5).
 *     For n > 4 this is the algebraic least-squares solution: cv2's Levenberg-Marquardt polish, RANSAC and LMedS are out.  The
 *     eigenvalue gap is not thresholded: three of four points exactly collinear are caught only by rule 6.
 *
 * skimi_homography_points: x [G, n, 2], H [G, 9] (dev; shared != 0: one H [9] for every group) -> out [G, n, 2].  w = (h6 x +
 * h7 y) + h8, X and Y alike; out = (X / w, Y / w), NaN in both coordinates when the input or w is non-finite or |w| < eps
 * (the reference raises there; a batch cannot).  G n <= 2^31; an empty call launches nothing.
 *
 * skimi_warp_perspective_u8 = cv2.warpPerspective(INTER_LINEAR, constant border 0): in [C, F, H, W, ch] u8 -> out [C, F, OH, OW,
 * ch] u8 (dev), ch 1, 3 or 4, sides 1 .. SKIMI_LENS_MAX_SIDE, C F <= 65535.  Hinv (DEV) [C, 9], or [C F, 9] when per_frame != 0,
 * maps output pixels to source positions: for output pixel (u, v), X = (g0 u + g1 v) + g2, Y and w alike, su = X / w, sv = Y / w
 * by plain division with no test of w's sign, as cv2: what lies beyond the horizon line is mirrored as cv2 mirrors it.  Then
 * rule 7 of the lens block verbatim (csrc/warp_u8.h is the one copy of it): 0 unless -1 < su < W and -1 < sv < H (any
 * non-finite value fails: a failed fit's NaN matrix gives a black frame), floor, a, b, taps outside count 0, the same
 * bilinear expression, floor(value + 0.5), the same stores.  cv2 quantises positions to 1/32 px with integer weights; this
 * rule is the contract.  The input is only read; nothing beyond the C F OH OW ch output bytes is written.
 *
 * skimi_bev_skeleton = project_world_to_bev_centered + the centre of merge: X [T, J, 3], center_px [T, 2] (dev) -> uv [T, J, 2]
 * f64, px [T, J, 2] i32, valid [T, J] u8, center_world [T, 3] (dev).  ax0, ax1 in 0 .. 2 (the reference's use_axes).
 *  1. center_world = np.nanmean over the joints PER COORDINATE (NaN skipped, an infinity is not); an all-NaN column: NaN.
 *     Lane l of the step's wave adds its joints l, l + 64, .. in order, then reduce.h's wave_sum.  center_world_in [T, 3]
 *     (dev, or NULL): the caller's centre, taken in place of the mean (project_world_to_bev_centered's own argument).
 *  2. A joint is valid iff its three coordinates, the two centre coordinates used and the step's center_px are finite.
 *  3. dx = x[ax0] - c[ax0], dz = x[ax1] - c[ax1], swapped when rot90_left != 0; du = dx / mpp, dv = -dz / mpp; (u0, v0) = rint
 *     of center_px; uv = (u0 + du, v0 + dv); px = rint(uv), rounding half to even as Python's round (saturating at int32).
 *  4. An invalid joint: NaN in uv, 0 in px.
 *
 * skimi_ground_track: p [P, T, 2] metres (dev), fps > 0 -> out [P, T, 6] = step, path, vx, vy, speed, heading.
 *  1. step_t = || p_t - p_(t-1) ||, 0 at t = 0, NaN if either end is non-finite.  path_t = the sum of the finite steps up to t,
 *     in time order (one thread per person).
 *  2. v_t = ((p_(t+1) - p_(t-1)) fps) / 2, one-sided (p_1 - p_0) fps and (p_(T-1) - p_(T-2)) fps at the ends; NaN in both
 *     components where a needed sample is non-finite or T = 1.  speed = || v ||, heading = atan2(vx, vy).
 *  3. Nothing is smoothed: callers smooth the track first. */
int skimi_homography_fit(const double* src, const double* dst, const double* post, int64_t G, int32_t n, double* H, double* Hinv,
                         double* Hn, double* err, double* stats, int32_t* status, void* stream);
int skimi_homography_points(const double* x, const double* H, int64_t G, int64_t n, int32_t shared, double eps, double* out,
                            void* stream);
int skimi_warp_perspective_u8(const uint8_t* in, uint8_t* out, const double* Hinv, int32_t per_frame, int32_t C, int32_t F,
                              int32_t H, int32_t W, int32_t OH, int32_t OW, int32_t ch, void* stream);
int skimi_bev_skeleton(const double* X, const double* center_px, const double* center_world_in, int64_t T, int32_t J,
                       double metres_per_pixel, int32_t ax0, int32_t ax1, int32_t rot90_left, double* uv, int32_t* px, uint8_t* valid,
                       double* center_world, void* stream);
int skimi_ground_track(const double* p, int64_t P, int64_t T, double fps, double* out, void* stream);

/* ---- camera calibration from the corners of a plane target: Zhang's start + Levenberg-Marquardt (csrc/calibrate.hip) ----
 * camera_calibration/main.py (cv2.calibrateCamera on chessboard corners, its prune step and standard deviations), corners
 * given as arrays.  obj [n, 2] (dev): the target's corners in its own plane (z = 0), shared by all boards; img [V, n, 2]
 * (dev) pixels; use [G, V] u8 (dev, or NULL: every view in every group); K0 [G, 3, 3] and dist0 [G, 12] (dev, or NULL);
 * width, height, free_mask (12 bits over fx fy cx cy k1 k2 p1 p2 k3 k4 k5 k6: bit i frees parameter i; dist's order is
 * the lens block's, so dist[0 .. 7] = parameters 4 .. 11 and dist[8 .. 11], the thin-prism terms, are always 0) and
 * max_evals are host scalars.  Each of the G groups is one calibration problem over the same V views under its own `use`
 * row, solved by one workgroup.  Everything is float64.  A call is the copy of obj once per board into the workspace, the
 * homography fit above on the V boards (shared by all groups) and the solver kernel: no host synchronisation, no
 * allocation, no atomics.  Every sum has a fixed order that depends only on (view, corner) indices: a group is bitwise what
 * it is alone, inside a batch and on a rerun.  Limits: 1 <= G <= 2^20 - 16, 1 <= V <= 1024, 4 <= n <= 4096; the workspace
 * is skimi_calibrate_workspace_bytes(G, V, n) bytes (0 for sizes the call refuses), 8-byte aligned.  Bad arguments:
 * SKIMI_ERR_ARG before any launch, outputs untouched.  Rules (DESIGN §2 "Calibration"; tests/calibrate_restated.py):
 *  1. Masks.  A corner is used iff its two image coordinates (and its two object coordinates) are finite.  A view is used in
 *     group g iff use[g, v] != 0, it has >= 4 used corners and its homography has status 1.  Fewer than 3 used views, or
 *     fewer residuals than parameters (2 x used corners < free intrinsics + 6 x used views), fails the group: every float
 *     output NaN, success 0, n_evals 0 (n_views and n_corners still count); its neighbours are untouched.  An unused view of
 *     a good group has NaN pose and NaN errors.
 *  2. Start of the intrinsics.  K0 NULL (cv2's initCameraMatrix2D): cx = (width - 1) / 2, cy = (height - 1) / 2; per used
 *     view, in view order, Hc = T Hn with T the translation by (-cx, -cy), h = column 0, v = column 1, d1 = (h + v) / 2,
 *     d2 = (h - v) / 2, each of the four scaled to unit length, giving the rows [h0 v0, h1 v1 | -h2 v2] and [d1_0 d2_0,
 *     d1_1 d2_1 | -d1_2 d2_2]; the 2 x 2 normal equations N (a, b) = r over all rows, det = N00 N11 - N01 N01, a = (N11 r0 -
 *     N01 r1) / det, b = (N00 r1 - N01 r0) / det; fx = sqrt|1 / a|, fy = sqrt|1 / b|.  K0 given (cv2's USE_INTRINSIC_GUESS):
 *     fx fy cx cy from K0.  The coefficients start at dist0[0 .. 7], or zero.  A zero or non-finite focal length, a non-finite
 *     principal point or coefficient fails the group.
 *  3. Start of each pose.  M = K^-1 Hn, negated when M22 < 0; s = 1 / ||M col 0||, r1 = s M col 0, r2 = s M col 1, r3 = r1 x
 *     r2, R = the nearest rotation to [r1 r2 r3] (csrc/svd3.h), t = s M col 2.
 *  4. Residual.  Xc = R (X, Y, 0) + t, (x, y) = Xc.xy / Xc.z, rule 2 of the lens block with s1 .. s4 = 0, r = (fx x_d + cx,
 *     fy y_d + cy) - corner.  cost = sum r^2 over the used corners of the used views: plain least squares, as cv2.
 *  5. Parameters.  The free intrinsics are additive; per view R <- Exp(w) R, t <- t + dt.  A fixed intrinsic keeps its start:
 *     its Jacobian column is zero and its row and column of the reduced system are the identity with a zero right side.
 *  6. Step (Marquardt's scaling, as cv2's CvLevMarq and MINPACK): (H + lam diag H) d = -g, H = J^T J from the analytic
 *     Jacobian, solved exactly through the Schur complement on the views: B*_v = B_v + lam diag B_v (6 x 6, LDL^T), S = A +
 *     lam diag A - sum_v C_v B*_v^-1 C_v^T (12 x 12), d_intr = S^-1 (-g_a + sum_v C_v B*_v^-1 g_v) by LDL^T without
 *     pivoting, d_v = -B*_v^-1 (g_v + C_v^T d_intr).  lam0 = 1e-3.
 *  7. Accept iff the trial's cost, evaluated from the trial parameters, is finite and <= c (1 + 1e-14): lam <- max(lam / 10,
 *     1e-16); else lam <- 10 lam and the step is solved again from the stored blocks.
 *  8. Stop on an accepted step with ||d|| <= 3e-8 (1 + ||x||) (success 1), d over the free intrinsics and every used view's
 *     (w, dt), x the free intrinsics and the used views' t after the step; on lam >= 1e30; after max_evals cost evaluations
 *     (the start and every trial count).
 *  9. Finish.  The blocks are re-linearised at the stopping point; S0 = the Schur complement at lam = 0; std[i] = sqrt((S0^-1)_ii
 *     cost / (m - p)) for the free intrinsics, m = 2 x used corners, p = free intrinsics + 6 x used views (cv2's
 *     stdDeviationsIntrinsics); NaN for a fixed intrinsic, where m <= p and where a factorisation
 *     (a view's B_v or S0) meets a pivot that is not positive.
 * 10. Outputs (dev): K [G, 3, 3], dist [G, 12], R [G, V, 3, 3], t [G, V, 3], rvec [G, V, 3] (cv2.Rodrigues of R), err [G, V, n]
 *     pixel distance (NaN where unused), view_stats [G, V, 3] = mean, rms, max, rms [G] = sqrt(cost / used corners) (cv2's
 *     return value), cost0, cost [G], std [G, 12] (free_mask's order), n_evals, n_views, n_corners, success [G] i32. */
size_t skimi_calibrate_workspace_bytes(int64_t G, int32_t V, int32_t n);
int skimi_calibrate_camera(const double* obj, const double* img, const uint8_t* use, const double* K0, const double* dist0, int64_t G,
                           int32_t V, int32_t n, int32_t width, int32_t height, int32_t free_mask, int32_t max_evals, double* K,
                           double* dist, double* R, double* t, double* rvec, double* err, double* view_stats, double* rms,
                           double* cost0, double* cost, double* std, int32_t* n_evals, int32_t* n_views, int32_t* n_corners,
                           int32_t* success, void* ws, size_t ws_bytes, void* stream);

/* ---- chessboard corners from whole frames: candidates and sub-pixel refinement (csrc/chessboard.hip) ----
 * camera_calibration/main.py:80-90 (find_chessboard_corners = cv2.findChessboardCorners + cv2.cornerSubPix), under the
 * project's own rules: OpenCV's quad-based detector (adaptive threshold, fast_check, its board-orientation heuristic) is
 * not restated.  frames [N, H, W, ch] u8 (dev), ch 1, 3 or 4, the layout of skimi_undistort_u8 with C F = N; 1 <= N <= 65535,
 * sides 1 .. SKIMI_LENS_MAX_SIDE, H W <= SKIMI_CHESS_MAX_PIXELS.  Integer stages are exact, the only atomics are integer
 * (order-independent), no host synchronisation, no allocation: results are bitwise reproducible and a frame's results are
 * the same bits alone and inside a batch.  The frames are only read.  Bad arguments: SKIMI_ERR_ARG before any launch.
 * Rules (DESIGN §2 "Chessboard corners"; tests/chessboard_restated.py):
 *  1. Gray.  ch 1: the byte.  ch 3 or 4: the channels in the order given are taken as B, G, R (the reference reads its
 *     frames with cv2), gray = (3735 B + 19235 G + 9798 R + 16384) >> 15; a fourth channel is ignored.
 *  2. Blur.  b = [1 2 1]^T [1 2 1] * gray, unnormalised (16 x the mean), int32.
 *  3. Response (ChESS, Bennett & Lasenby).  Ring offsets (dx, dy) = (rint(5 cos(k pi / 8)), rint(5 sin(k pi / 8))), k = 0 .. 15:
 *     (5,0) (5,2) (4,4) (2,5) (0,5) (-2,5) (-4,4) (-5,2) (-5,0) (-5,-2) (-4,-4) (-2,-5) (0,-5) (2,-5) (4,-4) (5,-2); I_k = b
 *     there.  SR = sum_{n<4} |I_n + I_{n+8} - I_{n+4} - I_{n+12}|, DR = sum_{n<8} |I_n - I_{n+8}|, MR = |5 sum_k I_k - 16 (b(0,0) +
 *     b(-1,0) + b(1,0) + b(0,-1) + b(0,1))|, R = 5 (SR - DR) - MR in int32.  R = 0 where x < 6, x >= W - 6, y < 6 or y >= H - 6.
 *     rmax [N] = the frame's maximum of R (>= 0: the border is part of the frame).
 *  4. Candidates.  A pixel is one iff R > 0, 256 R > threshold rmax in int64 (threshold in 1/256 units, 0 .. 256) and R is the
 *     maximum of its (2 nms_radius + 1)^2 window clipped to the frame (0 <= nms_radius <= SKIMI_CHESS_MAX_NMS): R > R' for
 *     every earlier pixel of the window in raster order, R >= R' for every later one.  A frame's candidates are written in
 *     ascending pixel order: xy [N, M, 2] i32 = (x, y), response [N, M] i32 = R, the first M = max_candidates of them; the
 *     rows behind them are (-1, -1) and 0.  count [N] i32 is the uncapped number.
 *  5. skimi_corner_subpix = cv2.cornerSubPix's iteration in float64 on any points [N, M, 2] f64 (dev) of those frames ->
 *     out [N, M, 2] f64, ok [N, M] u8.  count [N] i32 (dev, or NULL): only the first count[f] points of frame f are refined.
 *     Half window (wx, wy), 1 .. SKIMI_SUBPIX_MAX_WIN each; mask m(i, j) = exp(-((j - wx) / wx)^2) exp(-((i - wy) / wy)^2) for
 *     0 <= j <= 2 wx, 0 <= i <= 2 wy.  A round at (x, y): a = x - floor(x), b = y - floor(y); the patch p(r, c), 0 <= r < 2 wy + 3,
 *     0 <= c < 2 wx + 3, is the gray value (rule 1) at (floor(x) - wx - 1 + c + a, floor(y) - wy - 1 + r + b) = (1 - b) ((1 - a) g00
 *     + a g01) + b ((1 - a) g10 + a g11) with pixel coordinates clamped to the frame (replicated border); gx = p(i + 1, j + 2) -
 *     p(i + 1, j), gy = p(i + 2, j + 1) - p(i, j + 1) (no 1/2); gxx = (gx gx) m, gxy = (gx gy) m, gyy = (gy gy) m; A = sum gxx,
 *     B = sum gxy, C = sum gyy, bb1 = sum (gxx (j - wx) + gxy (i - wy)), bb2 = sum (gxy (j - wx) + gyy (i - wy)); lane l of the
 *     point's wave adds the window elements l, l + 64, .. (row-major) in order, then reduce.h's wave_sum.  det = A C - B B; zero
 *     or non-finite: the point stays where it is for good.  Else x += (C bb1 - B bb2) / det, y += (A bb2 - B bb1) / det; a point
 *     that is then not in [0, W) x [0, H) (a NaN fails) stops there, as cv2 stops.  Exactly `iters` rounds (0 ..
 *     SKIMI_SUBPIX_MAX_ITERS) and no epsilon stop, unlike cv2: an early stop would make two evaluations of the rule differ by a
 *     round near the threshold.  ok = the point was refined (inside its count, start finite and in [0, W) x [0, H)) and ended
 *     within (wx, wy) of its start, |dx| <= wx and |dy| <= wy; otherwise out = the start, as cv2 reverts it, and ok = 0.
 * Ordering the candidates into a board is host work on small arrays: calibration.order_chessboard. */
#define SKIMI_CHESS_MAX_PIXELS (1 << 28)
#define SKIMI_CHESS_MAX_NMS 15
#define SKIMI_SUBPIX_MAX_WIN 15
#define SKIMI_SUBPIX_MAX_ITERS 1000
size_t skimi_chess_workspace_bytes(int64_t N, int32_t H, int32_t W);
int skimi_chess_candidates(const uint8_t* frames, int64_t N, int32_t H, int32_t W, int32_t ch, int32_t threshold, int32_t nms_radius,
                           int32_t max_candidates, int32_t* xy, int32_t* response, int32_t* count, int32_t* rmax, void* ws,
                           size_t ws_bytes, void* stream);
int skimi_corner_subpix(const uint8_t* frames, int64_t N, int32_t H, int32_t W, int32_t ch, const double* points, const int32_t* count,
                        int32_t M, int32_t win_x, int32_t win_y, int32_t iters, double* out, uint8_t* ok, void* stream);

/* ---- ORB-style image features and Hamming matching (csrc/features.hip) ----
 * triangulation/camera_position/camera_position.py:181-226 (estimate_camera_pose_from_ORB = cv2.ORB_create +
 * cv2.BFMatcher(NORM_HAMMING, crossCheck)), under the project's own rules: OpenCV's keypoints, its learned BRIEF pattern and
 * its float orientation are not restated.  frames [N, H, W, ch] u8 (dev) as skimi_chess_candidates takes them.  Every stage is
 * integer arithmetic, the only atomics are integer, no host synchronisation, no allocation: results are bitwise reproducible
 * and a frame's (a set pair's) results are the same bits alone and inside a batch.  Bad arguments: SKIMI_ERR_ARG before any
 * launch.  Rules (DESIGN §2 "Image features"; tests/features_restated.py):
 *  1. Pyramid.  Level 0 = gray (rule 1 of the chessboard block).  L = levels, 1 .. SKIMI_ORB_MAX_LEVELS; level l has W_l =
 *     (2 W 5^l + 6^l) / (2 6^l), H_l likewise (integer division).  Level l from the unblurred level l - 1, per axis: n =
 *     (2 x + 1) W_{l-1} - W_l, den = 2 W_l, x0 = floor(n / den), a = ((n - x0 den) 256) / den, x0 and x0 + 1 clamped to the source;
 *     value = ((256 - ay) ((256 - ax) p00 + ax p01) + ay ((256 - ax) p10 + ax p11) + 2^15) >> 16.  Each level's blur: [1 4 6 4 1]^T
 *     [1 4 6 4 1] with replicated borders, (v + 128) >> 8.
 *  2. FAST score on the unblurred level.  Ring (dx, dy), k = 0 .. 15: (0,-3) (1,-3) (2,-2) (3,-1) (3,0) (3,1) (2,2) (1,3) (0,3)
 *     (-1,3) (-2,2) (-3,1) (-3,0) (-3,-1) (-2,-2) (-1,-3); d_k = ring_k - p.  s = max over the 16 arcs of 9 contiguous ring
 *     pixels of max(min_arc d, min_arc -d), 0 where that is negative and outside the candidate region: SKIMI_ORB_BORDER <= x <
 *     W_l - SKIMI_ORB_BORDER, the same for y.  A corner has s > threshold (0 .. 254).
 *  3. Keypoint candidates: corners whose s is the maximum of the 3 x 3 window, s > s' for the earlier pixels in raster order
 *     and s >= s' for the later ones; with roi [N, 4] f64 (x1, y1, x2, y2; or NULL) only those with x1 <= X < x2 and y1 <= Y < y2
 *     for the level-0 position (X, Y) of rule 7 (a NaN in the box fails).  level_count [N, L] = their number, uncapped.
 *  4. Harris on the unblurred level: Sobel Ix = (p(x+1,y-1) + 2 p(x+1,y) + p(x+1,y+1)) - (the same at x-1), Iy likewise; a, b, c
 *     = sum Ix^2, sum Iy^2, sum Ix Iy over the 7 x 7 block; h = 25 (a b - c^2) - (a + b)^2 in int64.
 *  5. Quota: w_l = 5^l 6^(L-1-l), q_l = floor(M w_l / sum w) for l >= 1, q_0 = M - sum of the others (M = max_features, 1 ..
 *     SKIMI_ORB_MAX_FEATURES).  Level l keeps its min(level_count, q_l) candidates of largest h, ties to the smaller pixel
 *     index.  Rows: levels in order, pixel order inside a level; count [N] = the kept number; the rows behind it hold -1 in
 *     xy_level, xy, level, direction and 0 in score, harris, desc.
 *  6. Orientation on the unblurred level: m10 = sum u I, m01 = sum v I over u^2 + v^2 <= 225; direction = the k in 0 .. 31 with
 *     the largest m10 C[k] + m01 S[k] (int64), ties to the smaller k; C = SKIMI_ORB_COS, S[k] = C[(k + 24) % 32].
 *  7. Descriptor, 256 bits: bit i = blur(p + a_i^k) < blur(p + b_i^k), in word i / 32 at position i % 32 of desc [N, M, 8] i32.
 *     pattern [32, 256, 4] i8 (dev) = (ax, ay, bx, by) for every direction: the base pattern is drawn with rule 3's splitmix64
 *     from s = SKIMI_ORB_PATTERN_SEED (no output discarded): four outputs give ax, ay, bx, by = (output mod 27) - 13; the draw
 *     is rejected unless ax^2 + ay^2 <= 169, bx^2 + by^2 <= 169, a != b and (a, b) was not drawn before; direction k holds
 *     ((x C[k] - y S[k] + 8192) >> 14, (x S[k] + y C[k] + 8192) >> 14) of both points.  The caller builds and uploads it.
 *     Outputs per row: xy_level [N, M, 2] i32; xy [N, M, 2] f64 = ((x + 0.5) W) / W_l - 0.5 (y with H); level, direction, score
 *     [N, M] i32; harris [N, M] i64.
 *  8. skimi_match_hamming: B pairs of descriptor sets d1 [B, M1, 8], d2 [B, M2, 8] i32 with n1, n2 [B] i32 (dev; clamped to 0
 *     .. M), M1, M2 <= SKIMI_ORB_MAX_FEATURES.  distance = popcount of the xor; for query i the nearest train j (ties: smaller
 *     j) and the second-nearest; for train j the nearest query (ties: smaller i).  Query i is kept iff n2 >= 1 and (cross_check
 *     == 0 or j's nearest query is i) and (ratio < 0 or (n2 >= 2 and (double)d_best < ratio (double)d_second)) and
 *     (max_distance < 0 or d_best <= max_distance).  The kept (i, j) ordered by (distance, i) (a stable counting sort); the
 *     first max_matches (1 .. SKIMI_ORB_MAX_FEATURES) go to pairs [B, max_matches, 2], dist [B, max_matches]; the rows behind
 *     hold -1; count [B] = the rows written. */
#define SKIMI_ORB_MAX_LEVELS 8
#define SKIMI_ORB_MAX_FEATURES 4096
#define SKIMI_ORB_BORDER 16
#define SKIMI_ORB_PATTERN_SEED 0x534B494D494F5242ULL
/* round(2^14 cos(2 pi k / 32)), k = 0 .. 31 */
#define SKIMI_ORB_COS                                                                                                          \
    {16384, 16069, 15137, 13623, 11585, 9102, 6270, 3196, 0, -3196, -6270, -9102, -11585, -13623, -15137, -16069, -16384, -16069, \
     -15137, -13623, -11585, -9102, -6270, -3196, 0, 3196, 6270, 9102, 11585, 13623, 15137, 16069}
/* round(2^14 sin(2 pi k / 32)), k = 0 .. 31 */
#define SKIMI_ORB_SIN                                                                                                          \
    {0, 3196, 6270, 9102, 11585, 13623, 15137, 16069, 16384, 16069, 15137, 13623, 11585, 9102, 6270, 3196, 0, -3196, -6270, -9102, \
     -11585, -13623, -15137, -16069, -16384, -16069, -15137, -13623, -11585, -9102, -6270, -3196}
size_t skimi_orb_workspace_bytes(int64_t N, int32_t H, int32_t W, int32_t levels);
int skimi_orb_features(const uint8_t* frames, int64_t N, int32_t H, int32_t W, int32_t ch, int32_t levels, int32_t threshold,
                       int32_t max_features, const double* roi, const int8_t* pattern, int32_t* xy_level, double* xy,
                       int32_t* level, int32_t* direction, int32_t* score, int64_t* harris, int32_t* desc, int32_t* count,
                       int32_t* level_count, void* ws, size_t ws_bytes, void* stream);
int skimi_match_hamming(const int32_t* d1, const int32_t* n1, int32_t M1, const int32_t* d2, const int32_t* n2, int32_t M2,
                        int64_t B, int32_t cross_check, double ratio, int32_t max_distance, int32_t max_matches, int32_t* pairs,
                        int32_t* dist, int32_t* count, void* stream);

/* ---- SIFT-style image features and L2 ratio-test matching (csrc/sift.hip) ----
 * triangulation/camera_position/camera_position.py:120-178, 242-297 (estimate_camera_pose_from_SIFT, estimate_pose_from_bbox_region
 * = cv2.SIFT_create + BFMatcher.knnMatch(k = 2) + Lowe's ratio test) under the project's own rules: parity with cv2.SIFT_create
 * is not pinned (no doubled first octave, one orientation per keypoint, the project's own sampling windows).  frames [N, H, W,
 * ch] u8 (dev) as skimi_orb_features takes them, the same limits on N, H, W.  A fixed number of launches for all frames (it
 * depends on `octaves` alone), no host synchronisation, no allocation, no float atomics; a frame's (a set pair's) results are
 * the same bits alone and inside a batch.  Bad arguments: SKIMI_ERR_ARG before any launch.  Rules (DESIGN §2 "Image features
 * (SIFT-style)"; tests/sift_restated.py):
 *  1. Gray = rule 1 of the chessboard block, converted to f32.
 *  2. Scale space in f32.  S = 3 intervals, sigma0 = 1.6, assumed input blur 0.5, no doubled first octave.  Octave o has 6
 *     Gaussian layers of size W_o x H_o, W_0 = W, W_{o+1} = (W_o + 1) / 2 (H likewise).  Layer 0 of octave 0 = gray blurred by
 *     sqrt(sigma0^2 - 0.25); layer i = layer i - 1 blurred by sigma0 2^((i-1)/S) sqrt(2^(2/S) - 1); layer 0 of octave o + 1 =
 *     layer S of octave o at even x and even y.  `octaves` = 0 .. SKIMI_SIFT_MAX_OCTAVES; an octave with min(W_o, H_o) < 16 is
 *     empty (the wrapper's default is the number of octaves that are not).  taps [6, 2 SKIMI_SIFT_MAX_RADIUS + 1] f32 (dev):
 *     row i holds the taps of layer i's blur, tap k of -r_i .. r_i at column SKIMI_SIFT_MAX_RADIUS + k, r_i = ceil(4 sigma_i)
 *     = SKIMI_SIFT_RADII[i]; the caller makes them in f64 (exp(-k^2 / (2 sigma_i^2)) normalised to sum 1), rounds them to f32
 *     and uploads them: no transcendental function runs on the device in this stage.  A blur = a horizontal pass, then a
 *     vertical pass over the f32 intermediate, borders replicated; each output = the f32 sum of f32 products added in tap
 *     order -r .. r, starting from the first product, unfused.  DoG layer i (0 .. 4) = layer i + 1 - layer i in f32.
 *  3. Candidates: a pixel of DoG layer 1 .. S with SKIMI_SIFT_BORDER <= x < W_o - SKIMI_SIFT_BORDER (y likewise), |d| >
 *     SKIMI_SIFT_PRETHRESH (f32) and d strictly greater than, or strictly smaller than, all 26 neighbours.  Compacted in
 *     (octave, layer, y, x) order; every (octave, layer) holds at most min(W_o H_o, SKIMI_SIFT_MAX_CANDIDATES) of them: those
 *     behind the capacity in (y, x) order are dropped.  octave_count [N, octaves] i32 = the candidates of an octave, uncapped.
 *  4. Refinement in f64 with + - * / only, unfused, on the f32 DoG values D.  Up to 5 rounds at (x, y, l): g = ((D(x+1) -
 *     D(x-1)) 0.5, the same in y, in l); dxx = D(x+1) + D(x-1) - 2 D, dyy, dss likewise; dxy = (D(x+1,y+1) - D(x-1,y+1) -
 *     D(x+1,y-1) + D(x-1,y-1)) 0.25, dxs, dys likewise; solve [dxx dxy dxs; dxy dyy dys; dxs dys dss] X = -g by elimination
 *     without pivoting in the order written in sift_refine (csrc/sift.hip) and tests/sift_restated.py.  A component of X
 *     > 0.5 moves x, y or l by + 1, < -0.5 by - 1; no move: settled.  A candidate that leaves the border or the layers 1 .. S,
 *     or has not settled in 5 rounds, is dropped.  response = D + ((g0 X0 + g1 X1) + g2 X2) 0.5; kept iff |response| >=
 *     SKIMI_SIFT_CONTRAST and det = dxx dyy - dxy dxy > 0 and (dxx + dyy)^2 10 < 121 det.  xy = ((x + X0) 2^o, (y + X1) 2^o);
 *     sigma = sigma0 2^o 2^(2/3) P(u ln 2), u = (l + X2) / 3 - 2/3, P = the Taylor polynomial of exp of degree 16 by
 *     Horner's rule (2^(2/3) = SKIMI_SIFT_CBRT4, ln 2 = SKIMI_SIFT_LN2); xy_level = (x, y), layer = l after the moves.
 *     With roi [N, 4] f64 (x1, y1, x2, y2; or NULL) only the keypoints with x1 <= xy.x < x2 and y1 <= xy.y < y2 stay.
 *  5. Selection: the max_features (1 .. SKIMI_SIFT_MAX_FEATURES) kept candidates of largest |response| (the bits of the
 *     f64 as an unsigned key, an exact radix selection), ties to the earlier candidate; rows in candidate order.  count [N]
 *     = their number; the rows behind it hold -1 in xy, xy_level, octave, layer, angle and 0 in sigma, response, desc.
 *  6. Orientation in f64 on Gaussian layer l of the octave, L: s = sigma / 2^o; samples at the integer offsets (i, j) from
 *     (x, y) with i^2 + j^2 <= (4.5 s)^2 whose pixel has all four neighbours; gx = L(x+1) - L(x-1), gy = L(y+1) - L(y-1);
 *     weight = sqrt(gx^2 + gy^2) exp(-(i^2 + j^2) / (2 (1.5 s)^2)); b = atan2(gy, gx) (into [0, 2 pi)) 36 / (2 pi); the vote
 *     goes to bins floor(b) and floor(b) + 1 (mod 36) with weights 1 - frac and frac.  Votes are added as integers of unit
 *     2^-43 (round to nearest; LDS integer adds, so the sum does not depend on the order).  Two circular [1 4 6 4 1] / 16
 *     smoothings; the highest bin k (ties: the smaller) with neighbours l, r: angle = 2 pi (k + 0.5 (l - r) / (l - 2 c + r))
 *     / 36 (no offset when the denominator is 0), into [0, 2 pi).  One orientation per keypoint: Lowe's secondary peaks >=
 *     0.8 are not emitted.
 *  7. Descriptor, 4 x 4 cells x 8 orientations, in f64: cell width h = 3 s; offsets (i, j), |i|, |j| <= R = floor(h sqrt(2) 2.5
 *     + 0.5), pixels with all four neighbours; c = (cos(angle) j + sin(angle) i) / h, r = (-sin(angle) j + cos(angle) i) / h
 *     (j along x, i along y); rb = r + 1.5, cb = c + 1.5, used iff -1 < rb < 4 and -1 < cb < 4; ob = (atan2(gy, gx) - angle)
 *     8 / (2 pi) into [0, 8); value = sqrt(gx^2 + gy^2) exp(-(r^2 + c^2) / 8); trilinear votes to the two nearest rows,
 *     columns (outside 0 .. 3: discarded) and orientations (mod 8), added as integers of unit 2^-43 as in rule 6.  v / |v|,
 *     min(., 0.2), / the new norm; desc [N, M, 128] u8, entry (row 4 + column) 8 + orientation = min(255, round half even
 *     (512 v)).
 *  8. skimi_match_l2: B pairs of descriptor sets d1 [B, M1, 128], d2 [B, M2, 128] u8 with n1, n2 [B] i32 (dev; clamped to 0 ..
 *     M), M1, M2 <= SKIMI_SIFT_MAX_FEATURES.  Exact i32 squared distances |a|^2 + |b|^2 - 2 a.b; for query i the nearest train j
 *     and the second-nearest by (distance, index): s1, s2 (s2 = -1 without a second train row); for train j the nearest query.
 *     Query i is kept iff n2 >= 1 and (cross_check == 0 or j's nearest query is i) and (ratio < 0 or (n2 >= 2 and (double)s1 <
 *     (ratio ratio) (double)s2)) and (max_distance2 < 0 or s1 <= max_distance2).  The kept (i, j) ordered by (s1, i) (a stable
 *     radix sort); the first max_matches (1 .. SKIMI_SIFT_MAX_FEATURES) go to pairs [B, max_matches, 2], dist2, second2 [B,
 *     max_matches] i32; the rows behind hold -1; count [B] = the rows written.  ws: 16-byte aligned, ws_bytes >= 8 B (M1 + M2)
 *     + 4 B M1. */
#define SKIMI_SIFT_MAX_OCTAVES 8
#define SKIMI_SIFT_MAX_FEATURES 4096
#define SKIMI_SIFT_MAX_CANDIDATES 32768
#define SKIMI_SIFT_BORDER 5
#define SKIMI_SIFT_MIN_SIDE 16
#define SKIMI_SIFT_MAX_RADIUS 13
#define SKIMI_SIFT_RADII {7, 5, 7, 8, 10, 13}
#define SKIMI_SIFT_PRETHRESH 1.7f
#define SKIMI_SIFT_CONTRAST 3.4
#define SKIMI_SIFT_CBRT4 1.5874010519681994
#define SKIMI_SIFT_LN2 0.6931471805599453
size_t skimi_sift_workspace_bytes(int64_t N, int32_t H, int32_t W, int32_t octaves);
int skimi_sift_features(const uint8_t* frames, int64_t N, int32_t H, int32_t W, int32_t ch, int32_t octaves, int32_t max_features,
                        const double* roi, const float* taps, double* xy, int32_t* xy_level, int32_t* octave, int32_t* layer,
                        double* sigma, double* response, double* angle, uint8_t* desc, int32_t* count, int32_t* octave_count,
                        void* ws, size_t ws_bytes, void* stream);
int skimi_match_l2(const uint8_t* d1, const int32_t* n1, int32_t M1, const uint8_t* d2, const int32_t* n2, int32_t M2, int64_t B,
                   int32_t cross_check, double ratio, int32_t max_distance2, int32_t max_matches, int32_t* pairs, int32_t* dist2,
                   int32_t* second2, int32_t* count, void* ws, size_t ws_bytes, void* stream);

/* ---- drawing into uint8 frame clips: discs, rings, capsules and 5 x 7 glyphs (csrc/draw.hip) ----
 * The last act of the reference's stages (cv2.circle / cv2.line / cv2.putText over every frame and joint), as one launch over
 * a clip.  frames, out [C, F, H, W, ch] u8 (dev), ch 1, 3 or 4, sides 1 .. SKIMI_LENS_MAX_SIDE, 1 <= C, F, C F <= 65535; out ==
 * frames draws in place, otherwise out receives every byte and frames is only read.  shapes (dev) i32 records of 8 words,
 * P <= SKIMI_DRAW_MAX_SHAPES a list: shape_axes 2: [P, 8] shared by every frame, 3: [F, P, 8] (frame f of every camera
 * reads list f), 4: [C, F, P, 8].  P = 0: out is a copy.  font (dev) u8 [96, 7]: characters 0x20 .. 0x7F, seven rows each, bit c
 * of a row byte = column c from the left (values < 32); the kernel holds no table.  The anti-aliasing and the font are THIS
 * PROJECT'S rules: no pixel parity with cv2's LINE_AA or Hershey fonts is claimed.  All arithmetic is integer; the result is
 * bitwise reproducible and bitwise that of tests/draw_restated.py.
 *  1. Record = kind, x0, y0, x1, y1, r, colour, opacity.  Positions and radii in 1/16 pixel; the centre of pixel (u, v) is
 *     (16 u, 16 v) (cv2's convention: integer coordinates are pixel centres).  x0, y0, r, and x1, y1 of kinds 1 .. 3, are
 *     saturated to +-2^20 on read (so no 64-bit expression below overflows); opacity is clamped to 0 .. 256; colour =
 *     0x00c2c1c0: channel i of the frame gets byte i, a 1-channel frame byte 0, channel 3 of a 4-channel frame is never written.
 *  2. Coverage cov in 0 .. 16 of a pixel centre p; isqrt = the exact floor square root of an int64; a = (x0, y0), b = (x1, y1).
 *     kind 0 (and any kind outside 0 .. 4): nothing.
 *     kind 1, disc: d = isqrt(|p - a|^2), cov = clamp(r + 8 - d, 0, 16).
 *     kind 2, ring of radius r and half thickness h = x1: cov = clamp(h + 8 - |d - r|, 0, 16).
 *     kind 3, capsule a -> b of half width r: a = b: the disc.  Else t = (p - a).(b - a), L2 = |b - a|^2; d = isqrt(|p - a|^2)
 *       if t <= 0, isqrt(|p - b|^2) if t >= L2, else |cross(p - a, b - a)| / isqrt(L2) (floor division); cov as the disc.
 *     kind 4, glyph: character x1 (outside 0x20 .. 0x7F: 0x7F), scale s = max(r, 1), cell top-left at pixel (left, top) =
 *       (floor(x0 / 16), floor(y0 / 16)), 5 s x 7 s pixels; cov = 16 where bit (u - left) / s of font row (v - top) / s is set,
 *       else 0: glyphs are not anti-aliased.
 *  3. Compositing per pixel and channel, in list order (painter's algorithm): a = cov opacity (0 .. 4096), value = (value
 *     (4096 - a) + colour_c a + 2048) >> 12; a = 0 changes nothing.  One thread owns a pixel: no atomics.
 *  4. A workgroup owns a block of 4 x 4 tiles of 64 x 16 pixels of one frame and composites on a tile only the shapes whose
 *     extent, grown by the radius (ring: r + h) plus one pixel, meets the tile; which shapes those are cannot change a byte
 *     (cov = 0 outside that box).  One launch, no workspace, no host synchronisation. */
#define SKIMI_DRAW_MAX_SHAPES 1024
#define SKIMI_DRAW_NONE 0
#define SKIMI_DRAW_DISC 1
#define SKIMI_DRAW_RING 2
#define SKIMI_DRAW_CAPSULE 3
#define SKIMI_DRAW_GLYPH 4
int skimi_draw_shapes_u8(const uint8_t* frames, uint8_t* out, const int32_t* shapes, int32_t shape_axes, const uint8_t* font,
                         int32_t C, int32_t F, int32_t H, int32_t W, int32_t ch, int32_t P, void* stream);

/* ---- 3D scene views: depth-buffered point splats and primitives (csrc/scene_view.hip) ----
 * What the reference's 3D stages end with (SceneVisualizer.draw_scene, vggt_camera_vis.py, the Open3D bird's-eye video), on
 * the device: clouds of coloured points and a list of depth-tested primitives (bones, joints, camera frusta, axes, grid
 * lines) seen from F cameras, one depth test per pixel.  frames u8 [F, H, W, 3] (dev), sides 1 .. SKIMI_LENS_MAX_SIDE.  THIS
 * PROJECT'S rules: no pixel parity with matplotlib or Open3D is claimed.  Depth is one integer per fragment, so the test is
 * exact; the result is bitwise reproducible, independent of the order of execution, and bitwise that of
 * tests/scene_view_restated.py.  Every f64 expression below is evaluated in the written order, without contraction.
 *  1. views f64 [F, 20] (dev): r00 r01 r02 t0, r10 r11 r12 t1, r20 r21 r22 t2 (world -> camera), fx, fy, cx, cy, near, far,
 *     ortho (non-zero: orthographic), one pad.  A point (x, y, z) f32 of the frame's cloud, as f64: X = ((r00 x + r01 y) +
 *     r02 z) + t0, Y and Z alike.  It is a fragment iff X, Y, Z are finite, near <= Z <= far, and (perspective) Z > 0.
 *     Perspective: u = (fx X) / Z + cx, v = (fy Y) / Z + cy, q = floor((2^30 near) / Z).  Orthographic: u = fx X + cx, v = fy Y +
 *     cy, q = floor((2^30 (far - Z)) / (far - near)).  w = q clamped to 1 .. 2^30 (a NaN gives 1): larger w is nearer, 0 is
 *     "empty".  Its pixel is (floor(u), floor(v)); with point_size s (1 .. SKIMI_SCENE_MAX_POINT_SIZE) it covers the s x s
 *     pixels from (floor(u) - (s - 1) / 2, floor(v) - (s - 1) / 2) (integer division), those inside the frame.
 *  2. Clouds: xyz f32 [P, N, 3], rgb u8 [P, N, 3] (dev), N < 2^31; count i64 [P] (dev) or NULL: cloud p holds min(max(count[p],
 *     0), N) points and the rows behind them are never read (a SceneCloud leaves them unwritten); the count is read by the
 *     kernel.  cloud_of_frame i32 [F] (dev) or NULL (then P == 1: cloud 0, or P == F: the frame's index); an entry outside
 *     0 .. P - 1 draws no cloud.  Splat pass: a thread per (frame, point) writes the key (w << 32) | point index into the
 *     workspace [F, H, W] u64 with a 64-bit atomic max: per pixel the nearest point wins, among equal w the highest index.
 *  3. prims i32 records of 12 words (dev), M <= SKIMI_SCENE_MAX_PRIMS a list; prim_axes 2: [M, 12] shared by every frame, 3:
 *     [F, M, 12].  Record = kind, x0, y0, x1, y1, r, colour, w0, w1, three reserved words (not read).  kind 1: disc at a = (x0,
 *     y0) with depth w0 (x1, y1, w1 not read); kind 2: capsule a -> b = (x1, y1) with depths w0 at a, w1 at b; any other kind:
 *     nothing.  Positions and r in 1/16 pixel, the centre of pixel (u, v) is (16 u, 16 v), saturated to +-2^20 on read; w0, w1
 *     clamped to 1 .. 2^30; colour 0x00c2c1c0 as skimi_draw_shapes_u8.  Coverage is hard, no anti-aliasing: the pixel centre p
 *     is covered iff d <= r with d the integer distance of skimi_draw_shapes_u8's rule 2 (disc; capsule with a = b: the disc).
 *     The fragment's depth: the disc's w0; the capsule's, with t = (p - a).(b - a), L2 = |b - a|^2: w0 if t <= 0, w1 if t >= L2,
 *     else w0 + sign(w1 - w0) floor(|w1 - w0| t / L2), exact (linear in w along the segment at the clamped foot of p: linear
 *     in inverse depth is perspective-correct).
 *  4. Resolve pass, one owner per pixel, no atomics: the pixel starts from its splat key (or empty); the primitives that
 *     cover it are visited in list order and one is taken iff its w >= the w held (so a primitive beats a point of equal w,
 *     and a later primitive an earlier one of equal w).  frames gets rgb[cloud, index] for a point, the record's colour for a
 *     primitive, else the background: background u8 [F, H, W, 3] (dev) or, when NULL, bg_colour (0x00c2c1c0).  depth f32 [F,
 *     H, W] or NULL: (float) of Z = (2^30 near) / w (perspective), far - (w (far - near)) / 2^30 (orthographic) of the w that
 *     won; +inf on an empty pixel.  index i32 [F, H, W] or NULL: the nearest POINT's index whatever primitives cover it, -1
 *     where no point landed (the cloud's visibility map from that camera).  Tiles and the two-level ordered binning of the
 *     list are skimi_draw_shapes_u8's rule 4; a tile that no primitive touches only resolves.
 *  5. ws (dev): 8 H W bytes a frame.  skimi_scene_view_workspace_bytes(F, H, W, cap_bytes) = 8 H W min(F, max(1, cap_bytes / (8
 *     H W))) (cap_bytes 0: no cap).  The call renders min(F, ws_bytes / (8 H W), 65535) frames at a time: per chunk one
 *     hipMemsetAsync, the splat launch (none when N == 0) and the resolve launch, all on `stream`: the number of launches
 *     depends on the shapes only.  ws smaller than one frame: SKIMI_ERR_WORKSPACE.  No host synchronisation. */
#define SKIMI_SCENE_MAX_PRIMS 1024
#define SKIMI_SCENE_MAX_POINT_SIZE 4
#define SKIMI_SCENE_NONE 0
#define SKIMI_SCENE_DISC 1
#define SKIMI_SCENE_CAPSULE 2
#define SKIMI_SCENE_W_ONE (1 << 30)
size_t skimi_scene_view_workspace_bytes(int64_t F, int32_t H, int32_t W, size_t cap_bytes);
int skimi_scene_view_render(const double* views, const float* xyz, const uint8_t* rgb, const int64_t* count,
                            const int32_t* cloud_of_frame, int32_t P, int64_t N, int32_t point_size, const int32_t* prims,
                            int32_t prim_axes, int32_t M, const uint8_t* background, uint32_t bg_colour, uint8_t* frames, float* depth,
                            int32_t* index, int64_t F, int32_t H, int32_t W, void* ws, size_t ws_bytes, void* stream);

/* ---- mask analysis: components, distance transform, boxes, IoU, greedy NMS (csrc/masks.hip) ----
 * The mask post-processing of the reference's SAM3 (perflib/connected_components.py, perflib/nms.py, perflib/masks_ops.py,
 * model/edt.py), on device masks.  A mask is u8 [H, W] (dev), non-zero = foreground; masks [B, H, W] with 1 <= H, W <=
 * SKIMI_MASK_MAX_SIDE and B H W < 2^31.  All arithmetic is integer (dist and iou are one stated float operation on integers);
 * every result is bitwise reproducible, bitwise that of tests/masks_restated.py, and for each mask what it is for that mask
 * alone.  No call synchronises or reads back, and the number of launches of a call depends on the shapes only.
 *  1. skimi_mask_components: connectivity 4 (the cross) or 8 (the full 3 x 3).  labels i32 [B, H, W]: 0 on background; the
 *     components of a mask are numbered 1 .. count[b] in the raster order of their first pixels (scipy.ndimage.label's
 *     numbering; THIS PROJECT'S rule: the reference's backends disagree with each other).  areas i32 [B, H, W]: the pixel count
 *     of the pixel's component, 0 on background.  count i32 [B].  stats i64 [B, max_components, 7] = area, x_min, y_min, x_max,
 *     y_max (inclusive), sum of x, sum of y of components 1 .. max_components; rows behind count[b] are zero; a component
 *     whose label is above max_components is missing from the table only.  max_components = 0: no table (stats may be NULL).
 *     ws (dev): skimi_mask_components_workspace_bytes.  Method: a block union-find (64 x 16 tiles in LDS, atomicMin across the
 *     tile borders); the root of a component is its smallest linear index, which no order of execution can change.
 *  2. skimi_mask_edt: d2 i32 [B, H, W] = the exact squared Euclidean distance from each pixel to the nearest zero pixel of its
 *     mask (0 on zero pixels); border_zero != 0: every position outside the image counts as zero (the reference's
 *     padding=True).  A mask without any zero (and border_zero = 0) gives d2 = SKIMI_EDT_NONE everywhere and dist = +inf (THIS
 *     PROJECT'S rule: the reference gives sqrt(1e18), cv2 a large finite value).  dist f32 [B, H, W] or NULL =
 *     (float)sqrt((double)d2).  Two integer passes: columns (vertical distance g), then rows (min over x' of (x - x')^2 +
 *     g(x')^2, stopped where (x - x')^2 + the row's smallest g^2 reaches the best so far).
 *  3. skimi_mask_argmax: of an i32 map [B, H, W] of values >= 0: xy i32 [B, 2] = (x, y) of the largest value, ties to the first
 *     in raster order; best i32 [B] = that value.
 *  4. skimi_mask_pack: masks [B, HW] -> words u64 [B, ceil(HW / 64)]: bit i of word k = pixel 64 k + i of the flattened mask, the
 *     last word zero-filled.  skimi_mask_boxes on packed masks: xyxy i32 [B, 4] = inclusive x_min, y_min, x_max, y_max; an empty
 *     mask gives (W, H, 0, 0) (the arithmetic of the reference's masks_to_boxes); area i32 [B].
 *  5. skimi_mask_iou: a [T, N, words], b [T, M, words] packed -> inter, uni i32 [T, N, M] = popcount(a & b), popcount(a | b),
 *     iou f32 = (float)inter / (float)max(uni, 1).  1 <= T <= 65535.
 *  6. skimi_nms_greedy: T problems; iou f32 [T, N, N], scores f32 [T, N], valid u8 [T, N] or NULL, N <= SKIMI_NMS_MAX -> keep
 *     u8 [T, N].  Entries are visited by score descending, ties (-0 = +0) to the lower index (THIS PROJECT'S rule: a stable
 *     sort, as the reference's Triton path; its CPU loop leaves ties to argsort); a visited entry that no kept entry
 *     suppressed is kept; a kept i suppresses every later j with iou[i, j] > iou_threshold (in f32; a NaN iou suppresses
 *     nothing).  An entry with valid == 0 or a NaN score is not kept and suppresses nothing.  One workgroup a problem. */
#define SKIMI_MASK_MAX_SIDE 4096
#define SKIMI_EDT_NONE (1 << 30)
#define SKIMI_NMS_MAX 1024
size_t skimi_mask_components_workspace_bytes(int64_t B, int32_t H, int32_t W);
int skimi_mask_components(const uint8_t* masks, int64_t B, int32_t H, int32_t W, int32_t connectivity, int32_t max_components,
                          int32_t* labels, int32_t* areas, int32_t* count, int64_t* stats, void* ws, size_t ws_bytes, void* stream);
int skimi_mask_edt(const uint8_t* masks, int64_t B, int32_t H, int32_t W, int32_t border_zero, int32_t* d2, float* dist, void* stream);
int skimi_mask_argmax(const int32_t* d2, int64_t B, int32_t H, int32_t W, int32_t* xy, int32_t* best, void* stream);
int skimi_mask_pack(const uint8_t* masks, int64_t B, int64_t HW, uint64_t* words, void* stream);
int skimi_mask_boxes(const uint64_t* words, int64_t B, int32_t H, int32_t W, int32_t* xyxy, int32_t* area, void* stream);
int skimi_mask_iou(const uint64_t* a, const uint64_t* b, int32_t T, int32_t N, int32_t M, int64_t words, float* iou, int32_t* inter,
                   int32_t* uni, void* stream);
int skimi_nms_greedy(const float* iou, const float* scores, const uint8_t* valid, int32_t T, int32_t N, float iou_threshold, uint8_t* keep,
                     void* stream);

/* ---- association and tracking: linear assignment, box tracker (csrc/assign.hip, csrc/lsap.h) ----
 * What the reference does on the host between frames (SAM3's perflib/associate_det_trk.py and model/sam3_video_base.py:
 * iou.cpu() + scipy.optimize.linear_sum_assignment; the same solver per time step in eval/hota_eval_toolkit) and what its
 * YOLO box picker says it lacks (prepare_dataset/model/yolov11_bbox.py: "no id-keeping mechanism").  One wave a problem / a
 * clip, no atomics, nothing read back, the launches of a call depend on the shapes only; every result is bitwise
 * reproducible, bitwise that of tests/assign_restated.py, and for each problem / clip what it is alone.
 *
 * skimi_linear_assignment: B problems; cost f64 [B, N, M] (dev), 1 <= N, M <= SKIMI_ASSIGN_MAX; n_rows, n_cols i32 [B] (dev)
 * or NULL (= N, M): problem b is the top-left n_rows[b] x n_cols[b] block (a count is clipped to 0 .. N, 0 .. M; 0 is an empty
 * problem).  -> row_to_col i32 [B, N], col_to_row i32 [B, M] (-1: unassigned; exactly min(n_rows, n_cols) pairs), total f64
 * [B], status i32 [B].  The minimum of the sum of the assigned costs; no forbidden edges.
 *  1. status = 1 iff the block holds a NaN or an infinity (or, with finite entries near the largest double, a step of the
 *     search finds no column at a finite distance): the maps are then all -1 and total is NaN.  Else status = 0.
 *  2. Method: shortest augmenting paths with dual variables u (rows), v (columns) in f64, all zero at the start (Crouse 2016,
 *     the method of scipy.optimize.linear_sum_assignment).  If n_rows > n_cols the transpose is solved.  Rows are inserted in
 *     ascending order.  For the row `cur` being inserted: min = 0, i = cur, every column unvisited with distance sp = +inf.
 *  3. A Dijkstra step: for every unvisited column j, r = ((min + cost[i, j]) - u[i]) - v[j]; if r < sp[j] then sp[j] = r and
 *     pred[j] = i.  The next column is the unvisited one with the smallest sp; TIES GO TO THE LOWEST COLUMN INDEX, with no
 *     preference for free columns.  min = its sp; it becomes visited; if it is free it is the sink, else i = its row.
 *  4. The duals after a path: u[cur] += min, and for every visited column j other than the sink u[row4col[j]] += min - sp[j]
 *     and v[j] -= min - sp[j] (row4col as it was before the path is flipped).  Then the path is flipped from the sink back
 *     along pred to cur.
 *  5. total = 0 + the assigned costs in ascending row order (of the block, not of the transpose), one f64 addition each.
 *  6. NOT PROMISED: scipy's assignment when the optimum is not unique.  scipy prefers a free column among equal distances and
 *     visits the columns in another order; where several assignments share the minimum the two may pick different ones (the
 *     totals agree to rounding).  With a unique optimum the assignment is scipy's.
 *
 * skimi_link_boxes: persistent ids for the boxes of B clips; boxes f64 [B, T, N, 4] (dev) x1, y1, x2, y2 in pixels, a box with
 * a non-finite coordinate is "no detection"; scores f64 [B, T, N] (dev) or NULL; 1 <= N, K <= SKIMI_LINK_MAX, K = the most
 * tracks a clip may have; max_age >= 0.  -> ids i32 [B, T, N] (-1: none), n_tracks i32 [B], table i32 [B, K, 3] = first frame,
 * last frame, hits of track k (-1, -1, 0 behind n_tracks), overflow i32 [B].  Frame by frame:
 *  1. The live tracks are those whose age is at most max_age, in ascending id order (age: the frames since the track was
 *     last matched; a track matched in frame t has age 0 at frame t + 1).  The detections are the valid boxes in index order.
 *  2. cost[d, k] = 1 - IoU(box d, the last box of live track k) in f64: iw = min(x2) - max(x1), ih = min(y2) - max(y1), inter =
 *     iw ih if both are > 0 else 0, union = (area_d + area_k) - inter, IoU = inter / union, 0 when union <= 0.  The rules of
 *     skimi_linear_assignment solve detections x live tracks (a failed solve assigns nothing).
 *  3. An assigned pair with IoU >= iou_threshold gives the detection the track's id, replaces the track's box and resets its
 *     age.  Every other valid detection with score >= new_score (no scores: every one) starts a track with the next id, in
 *     detection-index order.
 *  4. Ids are never reused.  When K tracks exist, further such detections get id -1 and overflow counts them.
 *  5. A track that was not matched in the frame ages by one. */
#define SKIMI_ASSIGN_MAX 1024
#define SKIMI_LINK_MAX 64
int skimi_linear_assignment(const double* cost, const int32_t* n_rows, const int32_t* n_cols, int64_t B, int32_t N, int32_t M,
                            int32_t* row_to_col, int32_t* col_to_row, double* total, int32_t* status, void* stream);
int skimi_link_boxes(const double* boxes, const double* scores, int64_t B, int32_t T, int32_t N, int32_t K, double iou_threshold,
                     int32_t max_age, double new_score, int32_t* ids, int32_t* n_tracks, int32_t* table, int32_t* overflow, void* stream);

/* ---- VGGT head and track-head helper kernels, one launch each ----
 * The kernels skimi_vggt_forward runs between its GEMMs, exposed singly so that each can be tested against a float64
 * restatement.  All maps are channels-last and dense; dtype / out_dtype are SKIMI_F32, SKIMI_BF16 or SKIMI_F16.  Every
 * call rejects null buffers, non-positive sizes and the shapes named below with SKIMI_ERR_ARG. */

/* F.interpolate(mode="bilinear", align_corners=True) of in [N, h, w, C] to out [N, H, W, C]; C % 4 == 0, N * H < 65536,
 * buffers 16-byte aligned.  Index arithmetic in float32 as ATen: scale = (in - 1) / (out - 1) (0 when out == 1), src =
 * scale * dst, i0 = min((int)src, in - 1), i1 = min(i0 + 1, in - 1), l1 = clamp(src - i0, 0, 1), l0 = 1 - l1;
 * v = l0y (l0x p00 + l1x p01) + l1y (l0x p10 + l1x p11) in fp32.  out_dtype < 0: the input's; else the input's, or
 * SKIMI_F32 from a 16-bit map.  tabx [W, C/2], taby [H, C/2] fp32 (both or neither, C % 8 == 0): v += c < C/2 ?
 * tabx[X][c] : taby[Y][c - C/2].  ln_g, ln_b [128] (both or neither; C == 128, fp32 out): every output pixel is then
 * LayerNorm'ed over its channels (two-pass variance, eps ln_eps) before it is stored. */
int skimi_resize_bilinear(const void* in, void* out, int32_t dtype, int32_t out_dtype, int32_t N, int32_t h, int32_t w,
                          int32_t H, int32_t W, int32_t C, const float* tabx, const float* taby, const float* ln_g,
                          const float* ln_b, float ln_eps, void* stream);
/* The same resize (+ tables) of an fp32 map written as bf16 halves hi = bf16(v), lo = bf16(v - hi) (round to nearest
 * even).  slice_records == 0: out [N, H, W, hi C | lo C], C % 16 == 0.  slice_records != 0: out [N, H, W, C/32,
 * hi 32 | lo 32], C % 32 == 0.  zpage (or NULL): 256 bytes that are cleared. */
int skimi_resize_bilinear_planes(const float* in, void* out, int32_t N, int32_t h, int32_t w, int32_t H, int32_t W,
                                 int32_t C, const float* tabx, const float* taby, int32_t slice_records, void* zpage,
                                 void* stream);
/* x [N, H, W, C] += c < C/2 ? tabx[X][c] : taby[Y][c - C/2] in place (sum in fp32, one rounding to x's type);
 * tabx [W, C/2], taby [H, C/2] fp32; C % 8 == 0. */
int skimi_add_uv_pos(void* x, int32_t dtype, const float* tabx, const float* taby, int32_t N, int32_t H, int32_t W,
                     int32_t C, void* stream);
/* The same sum of an fp32 x (tabx NULL: x alone), x left as it is, written as records rec [N * H * W, C/32, hi 32 |
 * lo 32] bf16 followed by 256 zero bytes (rec holds N * H * W * 2 C * 2 + 256 bytes); C % 32 == 0. */
int skimi_add_uv_pos_records(const float* x, const float* tabx, const float* taby, int32_t N, int32_t H, int32_t W,
                             int32_t C, void* rec, void* stream);
/* y[px][n] = sum_k in[px][k] W[n][k] + b[n], in [npix, 32], W [n_out, 32], n_out 2 or 4, fp32 accumulate in ascending k.
 * pts [npix, n_out - 1]: mode 0 exp(y), mode 1 sign(y) expm1(|y|); conf [npix] = 1 + exp(y[n_out - 1]). */
int skimi_dpt_out(const void* in, int32_t dtype, const float* W, const float* b, int32_t n_out, float* pts, float* conf,
                  int64_t npix, int32_t mode, void* stream);
/* img [F, 3, H, W] fp32 -> out [F * (H/p) * (W/p), Kp]: out[(f, py, px)][c p^2 + dy p + dx] = (img[f, c, py p + dy,
 * px p + dx] - mean[c]) / std[c] (ImageNet statistics), columns 3 p^2 .. Kp - 1 zero; Kp >= 3 p^2. */
int skimi_patch_gather(const float* img, void* out, int32_t out_dtype, int32_t F, int32_t H, int32_t W, int32_t p,
                       int32_t Kp, void* stream);
/* out = gate * (xn * (1 + scale) + shift) + x; xn, x, out [rows, D], mod [rows, shift D | scale D | gate D]. */
int skimi_adaln(const float* xn, const float* x, const float* mod, float* out, int64_t rows, int32_t D, void* stream);
/* pred = first ? delta : pred + delta on columns 0..8 of pred_pad [rows, 16] (columns 9..15 are left alone);
 * act_out [rows, 9] = pred with relu on columns 7 and 8; delta [rows, 9]. */
int skimi_pose_update(const float* delta, float* pred_pad, float* act_out, int64_t rows, int32_t first, void* stream);
/* x [F, P, C]: x[f, 0:n, :] = table[f % S == 0 ? 0 : 1][0:n, :], table [2, n, C]; rows n..P-1 are left alone. */
int skimi_special_tokens(float* x, const float* table, int32_t F, int32_t S, int32_t P, int32_t n, int32_t C, void* stream);

/* F.avg_pool2d(2, 2) of in [N, H, W, C] to out [N, H/2, W/2, C] (an odd last row / column is dropped). */
int skimi_track_avgpool2(const float* in, float* out, int32_t N, int32_t H, int32_t W, int32_t C, void* stream);
/* Bilinear sample (align_corners, border padding) of image b of fmap (images [H, W, C], img_stride floats apart,
 * img_stride >= H W C) at (x, y) = coords[(b N + n) coord_stride + 0 / 1] (coord_stride >= 2) -> out [B, N, C]. */
int skimi_track_sample_border(const float* fmap, int64_t img_stride, const float* coords, int64_t coord_stride, float* out,
                              int32_t B, int32_t N, int32_t H, int32_t W, int32_t C, void* stream);
/* One pyramid level of CorrBlock.corr_sample without the correlation volume: for row = (b, n, s) of rows = B N S,
 * out[row ldo + out_off + i (2r+1) + j] = <tgt[row], sample(fmap[b S + s])> / sqrt(C), sampled bilinearly (align_corners,
 * zeros padding) at (coords[row][0] / 2^level + i - r, coords[row][1] / 2^level + j - r): grid row i offsets x, column j
 * offsets y.  tgt [rows, C], fmap [B S, H, W, C], coords [rows, 2]; ldo >= out_off + (2r+1)^2. */
int skimi_track_corr_sample(const float* tgt, const float* fmap, const float* coords, float* out, int64_t rows, int32_t N,
                            int32_t S, int32_t H, int32_t W, int32_t C, int32_t r, int32_t level, int64_t ldo,
                            int32_t out_off, void* stream);
/* The 2D sin/cos position embedding of an H x W grid (get_2d_sincos_pos_embed, table values rounded to fp32) sampled
 * as skimi_track_sample_border does at coords[bn coord_stride + 0 / 1] -> out [BN, D]; D % 4 == 0: [sin x | cos x |
 * sin y | cos y], D/4 frequencies 1 / 10000^(k / (D/4)) each. */
int skimi_track_pos_embed_sample(const float* coords, int64_t coord_stride, float* out, int32_t BN, int32_t H, int32_t W,
                                 int32_t D, void* stream);
/* x[row] = [emb(flow) L | flow / max_scale, twice | fcorr[row] L | tfeat[row] L] + pos[bn] + qrt[s == 0 ? 0 : 1] for
 * row = (bn, s) of coords [rows, 2]; flow = coords[row] - coords[(bn, 0)]; emb = [x part L/2 | y part L/2], element
 * 2k sin(flow 2k (1000 / (L/2))), element 2k + 1 its cos.  pos [rows / S, 3L + 4], qrt [2, 3L + 4]; x has row stride
 * ldx >= 3L + 4 and its columns 3L + 4 .. ldx - 1 are written 0; L % 4 == 0. */
int skimi_track_input(const float* coords, const float* fcorr, const float* tfeat, const float* pos, const float* qrt,
                      float* x, int64_t rows, int32_t S, int32_t L, int64_t ldx, float max_scale, void* stream);
/* coords [rows, 2] += delta[row ldd + 0 / 1] (ldd >= 2), rows (b, n, s); rows with s == 0 are set to query[b, n]
 * instead.  pred (or NULL) [B, S, N, 2] = the new coords * stride. */
int skimi_track_coord_update(float* coords, const float* delta, int64_t ldd, const float* query, float* pred, int64_t rows,
                             int32_t N, int32_t S, float stride, void* stream);
/* coords [BN, S, 2] = q [BN, 2] * (1 / stride) for every s; qs [BN, 2] the same. */
int skimi_track_init(const float* q, float* coords, float* qs, int64_t BN, int32_t S, float stride, void* stream);
/* dst [BN, S, C] = src [BN, C] repeated over S. */
int skimi_track_repeat_rows(const float* src, float* dst, int64_t BN, int32_t S, int32_t C, void* stream);
/* out [B, S, N] = in [B, N, S]. */
int skimi_track_bns_to_bsn(const float* in, float* out, int32_t B, int32_t N, int32_t S, void* stream);

/* ---- VideoPose3D small-batch streaming layers, one launch each (csrc/vp3d_stream.hip, csrc/vp3d_dense.hip) ----
 * The kernels skimi_vp3d_forward runs below 2048 rows of its first layer, exposed singly so that every instantiation
 * can be tested against a float64 restatement.  Operands are bf16 hi / lo records, x = hi + lo with hi = bf16(x) and
 * lo = bf16(x - hi), round to nearest even, in fragment-major order:
 *     [row tile of 16][K slice of 32][hi | lo][kg 0..3][row 0..15][8 elements]           (2 KiB per tile and slice)
 * element (row, k) of the hi plane sits at 16-bit index ((row / 16) S + k / 32) 1024 + ((k % 32 / 8) 16 + row % 16) 8
 * + k % 8, S = K / 32, and its lo half 512 further.  Activation rows are b * Lin + l, weight rows output channels,
 * weight K = tap * C + channel.  Output records have the same layout with N in place of K (N % 32 == 0); rows past the
 * last of the last tile are unspecified.  A forced choice of 0 leaves that field to the planner; R and the row tiles
 * always follow from the planner's formulas, and a forced choice the planner could not have made feasible is refused
 * with SKIMI_ERR_ARG before anything is launched. */

/* w_host [N][K] fp32 on the host (K = taps * C, tap-major) -> dst, Npad * K * 4 bytes on the device, as weight records
 * with rows N .. Npad - 1 zero; Npad % 16 == 0, K % 32 == 0.  The code path of skimi_vp3d_finalize. */
int skimi_vp3d_pack_weights(const float* w_host, int32_t N, int32_t Npad, int32_t K, void* dst);
/* out[b Lout + l][n] = resid[(b resid_L + l + resid_off) C + n] + act(bias[n] + sum_t sum_c W[n][t C + c]
 * x[b Lin + l + t dil][c]), Lout = Lin - (taps - 1) dil, act = ReLU when relu != 0; resid may be NULL, else N == Npad ==
 * C.  out_f32 [B Lout][ldo] and / or out_rec (N % 32 == 0).  force_family 1: vp3d_conv_kernel (taps 1 or 3; force_nw 4
 * or 8, force_ms = row splits per clip), 2: vp3d_mm_kernel (force_ms = row splits of all B Lout rows); force_ct 16 or
 * 32; force_family 0 (then the other three 0 too): the production plan. */
int skimi_vp3d_stream_mm(const void* wrec, int32_t Npad, const void* xrec, const float* bias, const float* resid, int32_t resid_L,
                         int32_t resid_off, float* out_f32, int32_t ldo, void* out_rec, int32_t B, int32_t Lin, int32_t C,
                         int32_t taps, int32_t dil, int32_t N, int32_t relu, int32_t force_family, int32_t force_ct,
                         int32_t force_nw, int32_t force_ms, void* stream);
/* The window kernel of the dense model: the same sum at dilation 1, ReLU, no residual.  force_ta 1 or 2 (16 or 32
 * channels per workgroup), force_msc = row splits per clip.  Without a forced choice a layer whose window does not fit
 * the LDS goes to vp3d_mm_kernel, as in the forward. */
int skimi_vp3d_stream_win(const void* wrec, int32_t Npad, const void* xrec, const float* bias, float* out_f32, int32_t ldo,
                          void* out_rec, int32_t B, int32_t Lin, int32_t C, int32_t taps, int32_t N, int32_t force_ta,
                          int32_t force_msc, void* stream);
/* expand_conv: out[b Lout + l][c] = relu(bias[c] + sum_k W[c][k] x[(b Lin + l) Cin + k]), k < taps * Cin, x [B][Lin][Cin]
 * fp32, out_f32 [B Lout][C] and out_rec both written; C % 32 == 0.  valu == 0: the MFMA kernel, w = weight records
 * [C][ldw] with ldw = taps * Cin rounded up to 32 (zero padded), force_ms = row splits per clip.  valu != 0: the fp32
 * FMA kernel, w = fp32 [C][ldw] on the device, force_ms = row splits of all B Lout rows. */
int skimi_vp3d_stream_expand(const float* x, const void* w, int32_t ldw, const float* bias, float* out_f32, void* out_rec,
                             int32_t B, int32_t Lin, int32_t Cin, int32_t taps, int32_t C, int32_t valu, int32_t force_ms,
                             void* stream);
/* The plan of the calling thread's last streaming launch (a forward leaves its last layer's): out[0] family (1 conv,
 * 2 mm, 3 window, 4 MFMA expand, 5 VALU expand; 0: none yet), [1] channels per workgroup (CT, 16 TA, 32), [2] row tiles
 * RT (conv: halo included; VALU expand: 0), [3] the kernel's TAPS (conv; MFMA expand: 1) or the layer's taps, [4] waves
 * per workgroup, [5] row splits ms / msc, [6] rows per workgroup R, [7] workgroups.  A refused call leaves it as it was. */
void skimi_vp3d_last_plan(int32_t out[8]);

#ifdef __cplusplus
}
#endif
#endif /* SKIMI_H */
