// The attention launch of a packed [q | k | v] buffer, host code only: check -> plan -> launch.
//   check_attention(request)          every argument check, in one place, each message spelled once
//   plan_attention(request, switches) a pure function (no HIP call, no global, no getenv): which kernel family runs, on
//                                     which grid, in which output form -- the one place that decides it
//   attention_args(request, plan)     the kernels' AttnArgs
// and the launchers of attention_f32.hip, attention_x3.hip, attention_bf16.hip and attention_q64.hip, which take
// (AttnArgs, AttnPlan, stream) and only launch.  The calling thread's last launched plan is kept for
// skimi_attention_last_plan; a refused call leaves it as it was.
#include <math.h>

#include "common.h"
#include "env.h"
#include "kernels.h"

namespace skimi {

static thread_local AttnPlan tl_attn_plan = {};
void attention_set_last_plan(const AttnPlan& plan) { tl_attn_plan = plan; }
const AttnPlan& attention_last_plan() { return tl_attn_plan; }

// The switches, each in the class it always had (profiles/shared_mfma_helpers.md): SKIMI_ATTN_X3 and SKIMI_ATTN_MX are
// re-read per launch under SKIMI_ENV_DYNAMIC=1 (A/B timing, the tests' sweeps), the others once per process.
//   SKIMI_ATTN_X3=0      fp32 input: the exact-fp32 kernel even when scratch for the bf16x3 kernel is lent
//   SKIMI_ATTN_MX=0      SKIMI_PREC_FP8 quantises the bf16 output rows in a separate pass instead
//   SKIMI_ATTN_Q64=0     the first, 32-query-per-wave bf16 kernel (attention_bf16.hip)
//   SKIMI_ATTN_LDSPAD    bytes of unused dynamic LDS for the 64-query kernel: occupancy experiments, e.g. 65536 -> one
//                        workgroup per CU
//   SKIMI_ATTN_ABL       timing ablations (wrong results): only in a -DSKIMI_ABLATIONS build
static AttnSwitches attention_switches() {
    AttnSwitches s;
    s.x3 = (int)env_switch("SKIMI_ATTN_X3", 1);
    s.mx = (int)env_switch("SKIMI_ATTN_MX", 1);
    s.q64 = (int)env_once("SKIMI_ATTN_Q64", 1);
    s.ldspad = env_once("SKIMI_ATTN_LDSPAD", 0);
#ifdef SKIMI_ABLATIONS
    s.abl = (int)env_once("SKIMI_ATTN_ABL", 0);
#else
    s.abl = 0;
#endif
    return s;
}

AttnPlan plan_attention_f32(int batch, int heads, int seq_q, int head_dim) {
    AttnPlan p = {};
    p.family = ATTN_FAM_F32;
    p.hd = head_dim <= 64 ? 64 : 128;   // the split of d over lane halves needs head_dim <= HD with the upper half starting at HD/2
    p.queries = 128;
    p.grid = cdiv(seq_q, 128) * heads * batch;
    return p;
}

AttnPlan plan_attention(const AttnRequest& r, const AttnSwitches& s) {
    const long C = (long)r.heads * r.head_dim;
    if (r.dtype == SKIMI_F32) {
        AttnPlan p = plan_attention_f32(r.batch, r.heads, r.seq, r.head_dim);
        // fp32-accurate mode: the bf16x3 kernel (the same 128-query grid) when the caller lends scratch for the hi / lo planes
        if (s.x3 && r.head_dim == 64 && r.x3_scratch && r.x3_scratch_bytes >= attention_x3_scratch_bytes((long)r.batch * r.seq, 3 * C)) {
            p.family = ATTN_FAM_X3;
            if (r.want_records && ((uintptr_t)r.out & 127) == 0) p.out_form = ATTN_OUT_RECORDS;
            // only k and v are read as planes (q is split in registers), and they are the tail of the packed rows
            // [q | k | v]: the planes hold just those 2 C columns, k first
            p.c0 = C; p.pw = 2 * C; p.koff = 0; p.voff = C;
        }
        return p;
    }
    AttnPlan p = {};
    p.family = s.q64 ? ATTN_FAM_BF16_Q64 : ATTN_FAM_BF16_Q32;
    p.hd = 64;
    p.queries = s.q64 ? 256 : 128;
    p.grid = cdiv(r.seq, p.queries) * r.heads * r.batch;
    // MXFP8 rows: one head = two 32-channel blocks, each inside one lane pair of the 64-query kernel
    const bool mx = r.out_dtype == SKIMI_FP8MX && s.mx && r.dtype == SKIMI_BF16 && r.head_dim == 64 && r.heads % 2 == 0 && s.q64;
    p.out_form = mx ? ATTN_OUT_MX : r.out_dtype == SKIMI_F16 ? ATTN_OUT_F16 : ATTN_OUT_ROWS;
    p.q_prescaled = r.q_prescaled;
    p.lds_pad = s.q64 ? (int)s.ldspad : 0;
    // the ablations are variants of the plain launch: not of the padded one, nor of the 32-query kernel on prescaled q
    p.dbg = (s.q64 ? p.lds_pad != 0 : r.q_prescaled != 0) ? 0 : s.abl;
    return p;
}

bool attention_mx_output_ok(int dtype, int heads, int head_dim) {
    AttnRequest r = {};
    r.dtype = dtype;
    r.out_dtype = SKIMI_FP8MX;
    r.batch = r.seq = 1;
    r.heads = heads;
    r.head_dim = head_dim;
    return plan_attention(r, attention_switches()).out_form == ATTN_OUT_MX;
}

int check_attention_shape(const AttnArgs& a) {
    SKIMI_CHECK_ARG(a.q && a.k && a.v && (a.out || a.out_mx), "skimi_attention: null buffer");
    SKIMI_CHECK_ARG(a.batch > 0 && a.heads > 0 && a.seq_q > 0 && a.seq_k > 0, "skimi_attention: empty shape");
    return SKIMI_OK;
}

int check_attention(const AttnRequest& r) {
    SKIMI_CHECK_ARG(r.dtype == SKIMI_F32 || r.dtype == SKIMI_BF16, "skimi_attention: dtype must be SKIMI_F32 or SKIMI_BF16 (got %d)", r.dtype);
    if (r.out_dtype == SKIMI_FP8MX)
        SKIMI_CHECK_ARG(r.out && r.batch > 0 && r.seq > 0 && attention_mx_output_ok(r.dtype, r.heads, r.head_dim),
                        "skimi_attention: MXFP8 rows need bf16 q / k / v, head_dim 64 and an even number of heads");
    else
        SKIMI_CHECK_ARG(r.out_dtype == r.dtype || (r.dtype == SKIMI_BF16 && r.out_dtype == SKIMI_F16),
                        "skimi_attention: out_dtype is dtype, SKIMI_F16 or SKIMI_FP8MX for bf16 q / k / v (got %d -> %d)", r.dtype,
                        r.out_dtype);
    const AttnArgs a = attention_args(r, AttnPlan{});   // the streams and the shape: what the remaining checks look at
    if (r.dtype == SKIMI_F32) return check_attention_f32(a);   // null buffer, empty shape, head_dim: as the strided entry
    const int rc = check_attention_shape(a);
    if (rc) return rc;
    SKIMI_CHECK_ARG(r.head_dim == 64, "skimi_attention: the bf16 MFMA kernel is head_dim 64 only (got %d)", r.head_dim);
    // (k and v sit heads * 128 bytes and twice that behind q)
    SKIMI_CHECK_ARG(((uintptr_t)r.qkv & 15) == 0,
                    "skimi_attention: bf16 q / k / v are loaded in 16-B pieces: the buffer must be 16-B aligned");
    return SKIMI_OK;
}

AttnArgs attention_args(const AttnRequest& r, const AttnPlan& p) {
    AttnArgs a;
    const long C = (long)r.heads * r.head_dim;
    const size_t es = r.dtype == SKIMI_F32 ? 4 : 2;
    a.q = r.qkv;
    a.k = r.qkv ? (const char*)r.qkv + C * es : nullptr;
    a.v = r.qkv ? (const char*)r.qkv + 2 * C * es : nullptr;
    a.out = r.out;
    a.q_row = a.k_row = a.v_row = 3 * C;
    a.o_row = C;
    a.q_batch = a.k_batch = a.v_batch = (long)r.seq * 3 * C;
    a.o_batch = (long)r.seq * C;
    a.q_head = a.k_head = a.v_head = a.o_head = r.head_dim;
    a.batch = r.batch;
    a.heads = r.heads;
    a.seq_q = a.seq_k = r.seq;
    a.head_dim = r.head_dim;
    a.scale = 1.0f / sqrtf((float)r.head_dim);
    a.q_prescaled = p.q_prescaled;
    // the 32-query kernel multiplies by scale * log2(e): make that product 1
    if (p.family == ATTN_FAM_BF16_Q32 && p.q_prescaled) a.scale = 0.69314718055994530942f;
    a.out_f16 = p.out_form == ATTN_OUT_F16;
    if (p.out_form == ATTN_OUT_MX) {   // [token][align128(C)] payload + [token][align128(C) / 32] scales: gemm_fp8_launch's A operand
        a.out = nullptr;
        a.out_mx = r.out;
        a.mx_row = (long)align_up((size_t)C, 128);
        a.mx_srow = a.mx_row / 32;
        a.out_mx_scales = r.out_scales ? r.out_scales : (char*)r.out + (size_t)r.batch * r.seq * a.mx_row;
    }
    return a;
}

int attention_launch(const AttnRequest& r, hipStream_t st, int* out_records) {
    if (out_records) *out_records = 0;
    int rc = check_attention(r);
    if (rc) return rc;
    const AttnPlan p = plan_attention(r, attention_switches());
    SKIMI_CHECK_ARG(p.grid < (1l << 31), "skimi_attention: grid too large");
    const AttnArgs a = attention_args(r, p);
    if (p.family == ATTN_FAM_F32) {
        rc = attention_f32_launch(a, p, st);
    } else if (p.family == ATTN_FAM_X3) {
        rc = attention_x3_launch(a, p, r.x3_scratch, st);
    } else {
        const double bh = (double)a.batch * a.heads;
        rc = prof_bracket(prof_armed(PROF_ATTN_BF16, a.seq_k), st, 4.0 * bh * a.seq_q * (double)a.seq_k * 64.0,
                          2.0 * bh * 64.0 * (2.0 * a.seq_q + 2.0 * a.seq_k), [&] {
                              return p.family == ATTN_FAM_BF16_Q64 ? attention_q64_dispatch(a, p, st) : attention_bf16_launch(a, p, st);
                          });
    }
    if (rc) return rc;
    attention_set_last_plan(p);
    if (out_records) *out_records = p.out_form == ATTN_OUT_RECORDS;
    return SKIMI_OK;
}

}  // namespace skimi
