// Internal launch entry points shared between translation units of libskimi.
#pragma once
#include "common.h"

namespace skimi {

int gemm_dispatch(const skimi_gemm_desc* d, hipStream_t st, void* scratch, size_t scratch_bytes,
                  int force_splitk);

int layernorm_launch(const float* x, const float* x2, int64_t ldx, int64_t rows, int C,
                     const float* gamma, const float* beta, float eps, void* out, int out_dtype,
                     int64_t ldo, hipStream_t st, int64_t grp_rows = 0, int64_t grp_stride = 0,
                     int64_t grp_off = 0);
// out_dtype SKIMI_BF16X3_REC is written by the vector kernel only: C / 256 must be one of its instantiations
static inline bool layernorm_records_ok(int C) {
    return C % 256 == 0 && (C / 256 <= 4 || C / 256 == 6 || C / 256 == 8);
}

int qknorm_rope_launch(void* qkv, int dtype, int64_t tokens, int heads, const float* qn_w,
                       const float* qn_b, const float* kn_w, const float* kn_b, float eps,
                       const int32_t* pos, const float* rope_cos, const float* rope_sin, int rope_npos,
                       hipStream_t st, float q_scale = 1.f, int* q_scaled = nullptr);
// q_scale / q_scaled: the bf16 fast path can fold the softmax scale (x log2 e) into q BEFORE its one rounding
// to bf16 (attention_q64.hip then takes exp2 of the raw MFMA accumulator); *q_scaled says whether it did.

// general attention: q rows [batch, seq_q], k/v rows [batch, seq_k]; element strides
struct AttnArgs {
    const void* q;
    const void* k;
    const void* v;
    void* out;
    long q_row, k_row, v_row, o_row;        // stride between consecutive tokens
    long q_batch, k_batch, v_batch, o_batch;  // stride between batches
    long q_head, k_head, v_head, o_head;    // stride between heads
    int batch, heads, seq_q, seq_k, head_dim;
    float scale;
    // optional two-level batch (fp32 kernel only): batch index g = go * batch_inner + gi sits at
    // go * *_batch2 + gi * *_batch (batch_inner = 0: one level, offset g * *_batch)
    int batch_inner = 0;
    long q_batch2 = 0, k_batch2 = 0, v_batch2 = 0, o_batch2 = 0;
    int q_prescaled = 0;   // bf16 kernels: q already carries scale * log2(e) (qknorm_rope_launch's q_scale)
    int out_f16 = 0;       // bf16 kernels: the output rows are written as fp16 (proj's operand under SKIMI_PREC_F16)
    // 64-query kernel only (attention_mx_output_ok): the output rows as MXFP8 instead of `out` -- payload [token][mx_row]
    // e4m3 bytes, one E8M0 byte per 32 channels in [token][mx_srow] (proj's A operand under SKIMI_PREC_FP8)
    void* out_mx = nullptr;
    void* out_mx_scales = nullptr;
    long mx_row = 0, mx_srow = 0;
};

// attention.hip: the attention launch of a packed [q | k | v] buffer is check_attention -> plan_attention ->
// attention_args -> one launcher.  The calling thread's last launched plan is kept for skimi_attention_last_plan.
enum { ATTN_FAM_F32 = 1, ATTN_FAM_X3 = 2, ATTN_FAM_BF16_Q32 = 3, ATTN_FAM_BF16_Q64 = 4 };
enum { ATTN_OUT_ROWS = 0, ATTN_OUT_F16 = 1, ATTN_OUT_MX = 2, ATTN_OUT_RECORDS = 3 };
struct AttnRequest {
    const void* qkv;           // [batch * seq][3][heads][head_dim], dtype SKIMI_F32 or SKIMI_BF16
    void* out;                 // [batch * seq][heads * head_dim] rows of out_dtype; SKIMI_FP8MX: the e4m3 payload
                               // [batch * seq][Kp], Kp = heads * head_dim rounded up to 128 (gemm_fp8_launch's A operand)
    int dtype, out_dtype;      // out_dtype: dtype, SKIMI_F16 (bf16 input) or SKIMI_FP8MX (attention_mx_output_ok)
    int batch, seq, heads, head_dim;
    int q_prescaled;           // bf16 input: q already carries scale * log2(e) (qknorm_rope_launch's q_scale)
    void* x3_scratch;          // fp32 input, head_dim 64: >= attention_x3_scratch_bytes selects the bf16x3 kernel
    size_t x3_scratch_bytes;
    bool want_records;         // fp32 input: bf16x3 records (+ 256 zero bytes) in `out` where the plan allows
    void* out_scales;          // SKIMI_FP8MX, optional: the E8M0 scales [batch * seq][Kp / 32]; null: right behind the payload
};
struct AttnSwitches { int x3, mx, q64; long ldspad; int abl; };   // SKIMI_ATTN_X3, _MX, _Q64, _LDSPAD, _ABL
struct AttnPlan {
    int family;        // ATTN_FAM_*
    int hd;            // the exact-fp32 kernel's HD template argument (64 elsewhere)
    int queries;       // per workgroup
    long grid;         // workgroups
    int out_form;      // ATTN_OUT_*
    int q_prescaled;   // as honoured: bf16 kernels only
    int lds_pad;       // bytes of dynamic LDS (64-query kernel)
    int dbg;           // timing ablation (bf16 kernels, -DSKIMI_ABLATIONS builds)
    long c0, pw, koff, voff;   // bf16x3: the hi / lo planes hold columns c0 .. c0 + pw of the packed rows; k and v start at
                               // koff / voff inside a plane row
};
int check_attention(const AttnRequest& r);
AttnPlan plan_attention(const AttnRequest& r, const AttnSwitches& s);   // pure: no HIP call, no global, no getenv
AttnPlan plan_attention_f32(int batch, int heads, int seq_q, int head_dim);
AttnArgs attention_args(const AttnRequest& r, const AttnPlan& p);
// check, plan, launch; *out_records (may be null): whether bf16x3 records were written
int attention_launch(const AttnRequest& r, hipStream_t st, int* out_records = nullptr);
void attention_set_last_plan(const AttnPlan& plan);
const AttnPlan& attention_last_plan();
// the bf16 attention launch can write its output as MXFP8 (one head = two 32-channel blocks, each inside one lane pair):
// plan_attention's answer for this input under the current switches
bool attention_mx_output_ok(int dtype, int heads, int head_dim);
int check_attention_shape(const AttnArgs& a);   // null buffer, empty shape
// the launchers: (AttnArgs, AttnPlan, stream), no decision and no argument check of their own
int attention_f32_launch(const AttnArgs& a, const AttnPlan& p, hipStream_t st);
int attention_bf16_launch(const AttnArgs& a, const AttnPlan& p, hipStream_t st);   // attention_bf16.hip: 32 queries per wave
int attention_q64_dispatch(const AttnArgs& a, const AttnPlan& p, hipStream_t st);  // attention_q64.hip: 64 queries per wave
// attention_x3.hip: fp32-accurate attention (head_dim 64) on the bf16 matrix pipe, operands split hi + lo; `scratch`
// (>= attention_x3_scratch_bytes) takes the hi / lo planes of the k and v columns of the packed qkv buffer
size_t attention_x3_scratch_bytes(long tokens, long row_elems);
int attention_x3_launch(const AttnArgs& a, const AttnPlan& p, void* scratch, hipStream_t st);
// the exact-fp32 kernel on four separate streams (vggt_track.hip, skimi_attention_f32_strided; two-level batch): its own
// checks and plan_attention_f32
int check_attention_f32(const AttnArgs& a);
int attention_f32_launch(const AttnArgs& a, hipStream_t st);
// preprocess.hip: Pillow-exact separable uint8 resample pass, uint8 HWC -> fp32 CHW / 255 with crop / pad
int resample_u8_launch(const unsigned char* in, unsigned char* out, long outer, int n_in, int n_out, long inner,
                       const int* kk, const int* bounds, int ksize, hipStream_t st);
int u8_hwc_to_f32_chw_launch(const unsigned char* in, int H, int W, float* out, int OH, int OW, int y_off, int x_off,
                             float fill, hipStream_t st);
// conv_direct.hip: 3x3, Cin % 32 == 0 -> 32 channels, pad 1, fp32-accurate, on bf16 hi/lo planes
int conv_direct_pack_launch(const float* w, unsigned short* out, int Cin, hipStream_t st);
int conv_direct_n32_launch(const unsigned short* in_hi, const unsigned short* in_lo, const unsigned short* w_packed,
                           const float* bias, float* out, int F, int H, int W, int C, int relu, hipStream_t st,
                           long px_stride = 0);   // 0: separate planes [.., C]; 2C: pixel records [hi C | lo C]
// the same conv on the align-corners bilinear resize of src [F][h][w][C] fp32 to H x W (+ the UV embedding tabx [W][C/2],
// taby [H][C/2], or both null), interpolated in the window staging: bilinear_ac_planes_launch + conv_direct_n32_launch in
// one launch with the same bits.  Eligible: SKIMI_DPT_TAIL_FUSED != 0 and every window's source samples fit its staging.
bool conv_direct_n32_up_eligible(int h, int w, int H, int W, int C);
int conv_direct_n32_up_launch(const float* src, int h, int w, const float* tabx, const float* taby,
                              const unsigned short* w_packed, const float* bias, float* out, int F, int H, int W, int C, int relu,
                              hipStream_t st);

// VideoPose3D expand-conv im2col: x [B, L, Cin] f32 -> A0 [B*(L-k+1), Kpad] f32 (zero padded)
int vp3d_im2col_launch(const float* x, float* a0, int B, int L, int Cin, int k, int Kpad, hipStream_t st);

// gemm_fp8.hip: MXFP8 operands (e4m3 + E8M0 per 32 K) and the scaled-MFMA contraction
int quant_mx_launch(const void* x, int dtype, long ldx, long rows, int K, void* q, void* scales, hipStream_t st);
int gemm_fp8_launch(const void* A, const void* As, const void* W, const void* Ws, int M, int N, int K, const float* bias, int act,
                    const float* gamma, const float* resid, long ldr, void* out, int out_dtype, long ldo, hipStream_t st,
                    void* out_scales = nullptr);
// LayerNorm straight into MXFP8 (C a multiple of 256): payload [rows][C] e4m3 + scales [rows][C / 32]
bool gemm_fp8_mx_output_ok(int M, int N);   // gemm_fp8_launch accepts out_dtype SKIMI_FP8MX for this shape (bias + GELU epilogue)
int layernorm_mx_launch(const float* x, int64_t ldx, int64_t rows, int C, const float* gamma, const float* beta, float eps,
                        void* payload, void* scales, hipStream_t st);

// vp3d_stream.hip: the small-batch weight-streaming path of the TemporalModel (one launch per convolution).
// Every launcher is check -> plan -> launch: plan_vp3d_*() is a pure function of the layer's shape (and of the
// SKIMI_VP3D_TAPREUSE / SKIMI_VP3D_PAIRS switches) that names the kernel instantiation and its decomposition; the
// launch ladders take the plan.  The calling thread's last launched plan is kept for skimi_vp3d_last_plan.
enum { VP3D_FAM_CONV = 1, VP3D_FAM_MM = 2, VP3D_FAM_WIN = 3, VP3D_FAM_EXPAND_MFMA = 4, VP3D_FAM_EXPAND_VALU = 5 };
struct Vp3dPlan {
    int family;   // VP3D_FAM_*; 0 from plan_vp3d_win: no window fits, the layer goes to vp3d_mm_launch
    int ct;       // channels per workgroup: CT (conv, mm), 16 TA (win), 32 (expand)
    int rt;       // row tiles of 16 per workgroup, the halo included for conv (0: the VALU expand has none)
    int taps;     // the TAPS template argument (conv, MFMA expand: 1), else the layer's taps
    int nw;       // waves per workgroup
    int ms;       // row splits: per channel tile over all B * Lout rows (mm, VALU expand), per clip (conv, win, MFMA expand)
    int R;        // output rows per workgroup
    int grid;     // workgroups
    int lds;      // bytes of LDS per workgroup
};
// A forced choice (tests, A/B timing): a field that is 0 is the planner's.  R and RT always come from the planner's
// formulas, and a forced choice passes the planner's feasibility conditions or is refused with SKIMI_ERR_ARG.
struct Vp3dForce {
    int family;   // mm launcher: VP3D_FAM_CONV or VP3D_FAM_MM (0: plan everything, the other fields are ignored)
    int ct;       // mm launcher: CT 16 or 32; window launcher: TA 1 or 2
    int nw;       // conv family: 4 or 8
    int ms;       // ms / msc
};
int plan_vp3d_mm(int Npad, int B, int Lin, int C, int taps, int dil, const Vp3dForce* force, Vp3dPlan* plan);
int plan_vp3d_expand(int B, int Lin, int Cin, int taps, int C, int valu, int force_ms, Vp3dPlan* plan);
void vp3d_set_last_plan(const Vp3dPlan& plan);
const Vp3dPlan& vp3d_last_plan();
int vp3d_expand_launch(const float* x, const float* w, int ldw, const float* bias, float* out_f32, void* out_rec, int B, int Lin,
                       int Cin, int taps, int C, hipStream_t st, int force_ms = 0);
int vp3d_expand_mfma_launch(const float* x, const void* wfrag, int Kpad, const float* bias, float* out_f32, void* out_rec, int B,
                            int Lin, int Cin, int taps, int C, hipStream_t st, int force_ms = 0);
int vp3d_mm_launch(const void* wrec, int Npad, const void* xrec, const float* bias, const float* resid, int resid_L,
                   int resid_off, float* out_f32, int ldo, void* out_rec, int B, int Lin, int C, int taps, int dil, int N,
                   int relu, hipStream_t st, const Vp3dForce* force = nullptr);
// vp3d_dense.hip: TemporalModel(dense=True)'s wide dilation-1 convs at small batch (the tap-reuse window kernel)
bool vp3d_window_enabled();
int plan_vp3d_win(int Npad, int B, int Lin, int C, int taps, const Vp3dForce* force, Vp3dPlan* plan);
int vp3d_win_launch(const void* wrec, int Npad, const void* xrec, const float* bias, float* out_f32, int ldo, void* out_rec,
                    int B, int Lin, int C, int taps, int N, hipStream_t st, const Vp3dForce* force = nullptr);

}  // namespace skimi
