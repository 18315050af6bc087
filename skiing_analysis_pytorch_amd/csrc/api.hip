// C-ABI surface of libskimi.so: error channel, version, generic ops.
#include <stdarg.h>

#include <mutex>
#include <vector>

#include "common.h"
#include "gemm_epilogue.h"
#include "kernels.h"
#include "track_kernels.h"
#include "vggt_kernels.h"

namespace skimi {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int lds_opt_in(std::atomic<unsigned>& done, const void* kernel, int bytes, const char* what) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) {
        set_error("hipGetDevice failed (%s)", what);
        return SKIMI_ERR_HIP;
    }
    const unsigned bit = 1u << (dev & 31);
    if (done.load(std::memory_order_acquire) & bit) return SKIMI_OK;
    const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e != hipSuccess) {
        set_error("hipFuncSetAttribute(%s, %d bytes of LDS) failed: %s", what, bytes, hipGetErrorString(e));
        return SKIMI_ERR_HIP;
    }
    done.fetch_or(bit, std::memory_order_release);
    return SKIMI_OK;
}

struct ProfState {
    int kind = PROF_NONE;
    long min_key = 0;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pool;
    double flops = 0, bytes = 0;
    hipEvent_t pending = nullptr;
};
static ProfState g_prof;
// launches may come from several host threads (one per stream): the event list is shared, the
// bracket of a launch is found again through the launching thread's own index
static std::mutex g_prof_mu;
static thread_local size_t tl_prof_idx = 0;

bool prof_armed(int kind, long size_key) { return g_prof.kind == kind && size_key >= g_prof.min_key; }
void prof_before(hipStream_t st) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    std::pair<hipEvent_t, hipEvent_t> e;
    if (!g_prof.pool.empty()) {
        e = g_prof.pool.back();
        g_prof.pool.pop_back();
    } else {
        (void)hipEventCreate(&e.first);
        (void)hipEventCreate(&e.second);
    }
    (void)hipEventRecord(e.first, st);
    g_prof.ev.push_back(e);
    tl_prof_idx = g_prof.ev.size() - 1;
}
void prof_after(hipStream_t st, double flops, double bytes) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    if (tl_prof_idx >= g_prof.ev.size()) return;   // profile_stop ran in between
    (void)hipEventRecord(g_prof.ev[tl_prof_idx].second, st);
    g_prof.flops += flops;
    g_prof.bytes += bytes;
}

}  // namespace skimi

using namespace skimi;

extern "C" {

const char* skimi_last_error(void) { return g_err; }

int skimi_version(void) { return 100; }
int skimi_sizeof_gemm_desc(void) { return (int)sizeof(skimi_gemm_desc); }

int skimi_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int skimi_profile_start(int32_t kind, int64_t min_size) {
    SKIMI_CHECK_ARG(kind == PROF_ATTN_BF16 || kind == PROF_GEMM, "skimi_profile_start: unknown kernel kind %d", kind);
    for (auto& e : g_prof.ev) g_prof.pool.push_back(e);
    g_prof.ev.clear();
    g_prof.flops = g_prof.bytes = 0;
    g_prof.kind = kind;
    g_prof.min_key = min_size;
    return SKIMI_OK;
}

int skimi_profile_stop(double* total_ms, int64_t* launches, double* flops, double* bytes) {
    double ms = 0;
    for (auto& e : g_prof.ev) {
        SKIMI_HIP(hipEventSynchronize(e.second));
        float t = 0;
        SKIMI_HIP(hipEventElapsedTime(&t, e.first, e.second));
        ms += t;
    }
    if (total_ms) *total_ms = ms;
    if (launches) *launches = (int64_t)g_prof.ev.size();
    if (flops) *flops = g_prof.flops;
    if (bytes) *bytes = g_prof.bytes;
    for (auto& e : g_prof.ev) g_prof.pool.push_back(e);
    g_prof.ev.clear();
    g_prof.kind = PROF_NONE;
    return SKIMI_OK;
}

int32_t skimi_gemm_last_path(void) { return gemm_last_path(); }

int skimi_gemm(const skimi_gemm_desc* d, void* stream) {
    if (!d) {
        set_gemm_path(0, 0, 0, 0, 0);
        set_error("skimi_gemm: null descriptor");
        return SKIMI_ERR_ARG;
    }
    return gemm_dispatch(d, (hipStream_t)stream, d->splitk_scratch, (size_t)d->splitk_scratch_bytes,
                         d->force_splitk);
}

int skimi_resample_u8(const uint8_t* in, uint8_t* out, int64_t outer, int32_t n_in, int32_t n_out, int64_t inner,
                      const int32_t* kk, const int32_t* bounds, int32_t ksize, void* stream) {
    return resample_u8_launch(in, out, outer, n_in, n_out, inner, kk, bounds, ksize, (hipStream_t)stream);
}

int skimi_u8_hwc_to_f32_chw(const uint8_t* in, int32_t H, int32_t W, float* out, int32_t OH, int32_t OW, int32_t y_off,
                            int32_t x_off, float fill, void* stream) {
    return u8_hwc_to_f32_chw_launch(in, H, W, out, OH, OW, y_off, x_off, fill, (hipStream_t)stream);
}

int skimi_conv3x3_n32_pack(const float* w, void* packed, int32_t C, void* stream) {
    SKIMI_CHECK_ARG(w && packed && C > 0, "skimi_conv3x3_n32_pack: bad arguments");
    return conv_direct_pack_launch(w, (unsigned short*)packed, C, (hipStream_t)stream);
}

int skimi_conv3x3_n32(const void* in_hi, const void* in_lo, const void* packed_w, const float* bias, float* out,
                      int32_t F, int32_t H, int32_t W, int32_t C, int32_t relu, void* stream) {
    return conv_direct_n32_launch((const unsigned short*)in_hi, (const unsigned short*)in_lo,
                                  (const unsigned short*)packed_w, bias, out, F, H, W, C, relu, (hipStream_t)stream);
}

int skimi_conv3x3_n32_strided(const void* in_hi, const void* in_lo, const void* packed_w, const float* bias, float* out,
                              int32_t F, int32_t H, int32_t W, int32_t C, int32_t relu, int64_t px_stride, void* stream) {
    SKIMI_CHECK_ARG(px_stride > 0, "skimi_conv3x3_n32_strided: px_stride must be positive");
    return conv_direct_n32_launch((const unsigned short*)in_hi, (const unsigned short*)in_lo,
                                  (const unsigned short*)packed_w, bias, out, F, H, W, C, relu, (hipStream_t)stream,
                                  (long)px_stride);
}

int skimi_conv3x3_n32_upsampled(const float* src, int32_t h, int32_t w, const float* tabx, const float* taby,
                                const void* packed_w, const float* bias, float* out, int32_t F, int32_t H, int32_t W, int32_t C,
                                int32_t relu, void* rec, int32_t* fused, void* stream) {
    const bool up = conv_direct_n32_up_eligible(h, w, H, W, C);
    if (fused) *fused = up;
    if (up)
        return conv_direct_n32_up_launch(src, h, w, tabx, taby, (const unsigned short*)packed_w, bias, out, F, H, W, C, relu,
                                         (hipStream_t)stream);
    SKIMI_CHECK_ARG(rec != nullptr, "skimi_conv3x3_n32_upsampled: the two-launch path needs rec");
    const int rc = bilinear_ac_planes_launch(src, (unsigned short*)rec, F, h, w, H, W, C, (hipStream_t)stream, tabx, taby);
    if (rc != SKIMI_OK) return rc;
    return conv_direct_n32_launch((const unsigned short*)rec, (const unsigned short*)rec + C, (const unsigned short*)packed_w, bias,
                                  out, F, H, W, C, relu, (hipStream_t)stream, 2L * C);
}

int skimi_split_planes(const float* x, int64_t ld, int64_t rows, int32_t C, void* hi, void* lo, void* stream) {
    SKIMI_CHECK_ARG(x && hi && lo && rows > 0 && C > 0, "skimi_split_planes: bad arguments");
    return split_planes_launch(x, (long)ld, (long)rows, C, hi, lo, (hipStream_t)stream);
}

int skimi_split_records(const float* x, int64_t ld, int64_t rows, int32_t C, void* records, void* stream) {
    SKIMI_CHECK_ARG(x && records && rows > 0 && C > 0, "skimi_split_records: bad arguments");
    return split_records_launch(x, (long)ld, (long)rows, C, records, (hipStream_t)stream);
}

int skimi_dpt_fold_pack(const float* w_T, const float* b_T, const float* w_rn, int32_t C_in, int32_t C_mid, int32_t C_out,
                        int32_t s, void* w_records, float* beta, void* stream) {
    SKIMI_CHECK_ARG(w_T && w_rn && w_records && beta, "skimi_dpt_fold_pack: null buffer");
    SKIMI_CHECK_ARG(s >= 2 && s <= 16 && C_in > 0 && C_in % 32 == 0 && C_mid > 0 && C_out > 0, "skimi_dpt_fold_pack: bad sizes");
    float* tmp = nullptr;   // a pack-time call: it allocates its fp32 staging and waits for the stream
    SKIMI_HIP(hipMalloc((void**)&tmp, (size_t)(s + 2) * (s + 2) * C_out * C_in * 4));
    const int rc = dpt_fold_pack_launch(w_T, b_T, w_rn, C_in, C_mid, C_out, s, tmp, w_records, beta, (hipStream_t)stream);
    const hipError_t e = hipStreamSynchronize((hipStream_t)stream);
    (void)hipFree(tmp);
    if (rc) return rc;
    SKIMI_HIP(e);
    return SKIMI_OK;
}

int skimi_dpt_tap_sum(const float* taps, const float* bias, float* out, int32_t N, int32_t h, int32_t w, int32_t C, void* stream) {
    return dpt_tap_sum_launch(taps, bias, out, N, h, w, C, (hipStream_t)stream);
}

int skimi_quant_mx(const void* x, int32_t dtype, int64_t ldx, int64_t rows, int32_t K, void* payload, void* scales,
                   void* stream) {
    return quant_mx_launch(x, dtype, (long)ldx, (long)rows, K, payload, scales, (hipStream_t)stream);
}

int skimi_layernorm_mx(const float* x, int64_t ldx, int64_t rows, int32_t C, const float* gamma, const float* beta,
                       float eps, void* payload, void* scales, void* stream) {
    return layernorm_mx_launch(x, ldx, rows, C, gamma, beta, eps, payload, scales, (hipStream_t)stream);
}

int skimi_gemm_fp8(const void* A, const void* A_scales, const void* W, const void* W_scales, int32_t M, int32_t N,
                   int32_t K, const float* bias, int32_t act, const float* gamma, const float* resid, int64_t ldr,
                   void* out, int32_t out_dtype, int64_t ldo, void* out_scales, void* stream) {
    return gemm_fp8_launch(A, A_scales, W, W_scales, M, N, K, bias, act, gamma, resid, (long)ldr, out, out_dtype, (long)ldo,
                           (hipStream_t)stream, out_scales);
}

int skimi_layernorm(const float* x, const float* x2, int64_t ldx, int64_t rows, int32_t C,
                    const float* gamma, const float* beta, float eps, void* out, int32_t out_dtype,
                    int64_t ldo, void* stream) {
    return layernorm_launch(x, x2, ldx, rows, C, gamma, beta, eps, out, out_dtype, ldo,
                            (hipStream_t)stream);
}

int skimi_qknorm_rope(void* qkv, int32_t dtype, int64_t tokens, int32_t heads, const float* qn_w,
                      const float* qn_b, const float* kn_w, const float* kn_b, float eps,
                      const int32_t* pos, const float* rope_cos, const float* rope_sin,
                      int32_t rope_npos, void* stream) {
    return qknorm_rope_launch(qkv, dtype, tokens, heads, qn_w, qn_b, kn_w, kn_b, eps, pos, rope_cos,
                              rope_sin, rope_npos, (hipStream_t)stream);
}

// skimi_attention, skimi_attention_out, skimi_attention_ex: one request (kernels.h), one body (attention.hip)
static int attention_entry(const void* qkv, void* out, int32_t dtype, int32_t out_dtype, int32_t batch, int32_t seq, int32_t heads,
                           int32_t head_dim, int32_t q_prescaled, void* x3_scratch, uint64_t x3_scratch_bytes,
                           int32_t* out_records, void* stream) {
    AttnRequest r = {};
    r.qkv = qkv; r.out = out; r.dtype = dtype; r.out_dtype = out_dtype;
    r.batch = batch; r.seq = seq; r.heads = heads; r.head_dim = head_dim; r.q_prescaled = q_prescaled;
    r.x3_scratch = x3_scratch; r.x3_scratch_bytes = (size_t)x3_scratch_bytes;
    r.want_records = out_records != nullptr && *out_records != 0;
    return attention_launch(r, (hipStream_t)stream, out_records);
}

int skimi_attention(const void* qkv, void* out, int32_t dtype, int32_t batch, int32_t seq,
                    int32_t heads, int32_t head_dim, void* stream) {
    return attention_entry(qkv, out, dtype, dtype, batch, seq, heads, head_dim, 0, nullptr, 0, nullptr, stream);
}

int skimi_attention_out(const void* qkv, void* out, int32_t dtype, int32_t out_dtype, int32_t batch, int32_t seq,
                        int32_t heads, int32_t head_dim, void* stream) {
    return attention_entry(qkv, out, dtype, out_dtype, batch, seq, heads, head_dim, 0, nullptr, 0, nullptr, stream);
}

// the two calls of the block forward (vggt_block.hip), with its arguments, for kernel-level tests
int skimi_qknorm_rope_scaled(void* qkv, int32_t dtype, int64_t tokens, int32_t heads, const float* qn_w,
                             const float* qn_b, const float* kn_w, const float* kn_b, float eps,
                             const int32_t* pos, const float* rope_cos, const float* rope_sin,
                             int32_t rope_npos, float q_scale, int32_t* q_scaled, void* stream) {
    return qknorm_rope_launch(qkv, dtype, tokens, heads, qn_w, qn_b, kn_w, kn_b, eps, pos, rope_cos,
                              rope_sin, rope_npos, (hipStream_t)stream, q_scale, q_scaled);
}

int skimi_attention_ex(const void* qkv, void* out, int32_t dtype, int32_t out_dtype, int32_t batch, int32_t seq,
                       int32_t heads, int32_t head_dim, int32_t q_prescaled, void* x3_scratch,
                       uint64_t x3_scratch_bytes, int32_t* out_records, void* stream) {
    return attention_entry(qkv, out, dtype, out_dtype, batch, seq, heads, head_dim, q_prescaled, x3_scratch, x3_scratch_bytes,
                           out_records, stream);
}

void skimi_attention_last_plan(int32_t out[8]) {
    if (!out) return;
    const AttnPlan& p = attention_last_plan();
    const int32_t v[8] = {p.family, p.queries, p.out_form, p.q_prescaled, (int32_t)p.grid, p.hd, p.lds_pad, 0};
    for (int i = 0; i < 8; ++i) out[i] = v[i];
}

uint64_t skimi_attention_x3_scratch_bytes(int64_t tokens, int64_t row_elems) {
    return (uint64_t)attention_x3_scratch_bytes((long)tokens, (long)row_elems);
}

static inline bool is_elem_dtype(int32_t d) { return d == SKIMI_F32 || d == SKIMI_BF16 || d == SKIMI_F16; }
static inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// the LayerNorm launch of the DPT heads (vggt_dpt.hip) and the attention launch of the track head (vggt_track.hip's
// run_mha), with their arguments, for kernel-level tests.  The forward derives the gather and the strides itself; here
// what the kernels cannot notice is checked first.
int skimi_layernorm_ex(const float* x, const float* x2, int64_t ldx, int64_t in_rows, int64_t rows, int32_t C,
                       const float* gamma, const float* beta, float eps, void* out, int32_t out_dtype, int64_t ldo,
                       int64_t grp_rows, int64_t grp_stride, int64_t grp_off, void* stream) {
    SKIMI_CHECK_ARG(rows > 0 && in_rows > 0 && ldx >= 0, "skimi_layernorm_ex: rows, in_rows must be positive, ldx not negative");
    SKIMI_CHECK_ARG(grp_rows >= 0, "skimi_layernorm_ex: grp_rows = %ld is negative", (long)grp_rows);
    int64_t last = rows - 1;   // the largest input row read
    if (grp_rows > 0) {
        SKIMI_CHECK_ARG(grp_off >= 0 && grp_stride >= grp_off + grp_rows,
                        "skimi_layernorm_ex: the gather needs grp_off >= 0 and grp_stride >= grp_off + grp_rows (got %ld, %ld, %ld)",
                        (long)grp_rows, (long)grp_stride, (long)grp_off);
        last = (rows - 1) / grp_rows * grp_stride + grp_off + (rows - 1) % grp_rows;
    }
    SKIMI_CHECK_ARG(last < in_rows, "skimi_layernorm_ex: input row %ld is read, the input has %ld rows", (long)last, (long)in_rows);
    SKIMI_CHECK_ARG(out_dtype == SKIMI_BF16X3_REC || ldo >= C, "skimi_layernorm_ex: ldo = %ld is below C = %d", (long)ldo, C);
    return layernorm_launch(x, x2, ldx, rows, C, gamma, beta, eps, out, out_dtype, ldo, (hipStream_t)stream, grp_rows,
                            grp_stride, grp_off);
}

int skimi_attention_f32_strided(const float* q, const float* k, const float* v, float* out, const int64_t* q_strides,
                                const int64_t* k_strides, const int64_t* v_strides, const int64_t* o_strides,
                                int32_t batch, int32_t batch_inner, int32_t heads, int32_t seq_q, int32_t seq_k,
                                int32_t head_dim, float scale, void* stream) {
    SKIMI_CHECK_ARG(q_strides && k_strides && v_strides && o_strides, "skimi_attention_f32_strided: null stride list");
    SKIMI_CHECK_ARG(batch <= 65535 && heads <= 65535, "skimi_attention_f32_strided: batch %d and heads %d are grid dimensions (<= 65535)",
                    batch, heads);
    SKIMI_CHECK_ARG(batch_inner >= 0 && (batch_inner == 0 || batch % batch_inner == 0),
                    "skimi_attention_f32_strided: batch_inner %d must divide batch %d", batch_inner, batch);
    for (int i = 0; i < 4; ++i)
        SKIMI_CHECK_ARG(q_strides[i] % 4 == 0 && k_strides[i] % 4 == 0 && v_strides[i] % 4 == 0 && o_strides[i] % 4 == 0,
                        "skimi_attention_f32_strided: every stride must be a multiple of 4 elements (16-B loads)");
    SKIMI_CHECK_ARG(al16(q) && al16(k) && al16(v) && al16(out), "skimi_attention_f32_strided: 16-byte aligned buffers");
    AttnArgs a;
    a.q = q; a.k = k; a.v = v; a.out = out;
    a.q_row = q_strides[0]; a.k_row = k_strides[0]; a.v_row = v_strides[0]; a.o_row = o_strides[0];
    a.q_head = q_strides[1]; a.k_head = k_strides[1]; a.v_head = v_strides[1]; a.o_head = o_strides[1];
    a.q_batch = q_strides[2]; a.k_batch = k_strides[2]; a.v_batch = v_strides[2]; a.o_batch = o_strides[2];
    a.q_batch2 = q_strides[3]; a.k_batch2 = k_strides[3]; a.v_batch2 = v_strides[3]; a.o_batch2 = o_strides[3];
    a.batch = batch; a.batch_inner = batch_inner; a.heads = heads; a.seq_q = seq_q; a.seq_k = seq_k; a.head_dim = head_dim;
    a.scale = scale;
    return attention_f32_launch(a, (hipStream_t)stream);   // its own checks: null buffers, empty shape, head_dim
}

// ---- VGGT head / track-head helper kernels, one launch each (vggt_kernels.hip, track_kernels.hip): the forward
// calls the launches directly with sizes it derived itself; here every scalar a caller supplies is checked first ----

int skimi_resize_bilinear(const void* in, void* out, int32_t dtype, int32_t out_dtype, int32_t N, int32_t h, int32_t w,
                          int32_t H, int32_t W, int32_t C, const float* tabx, const float* taby, const float* ln_g,
                          const float* ln_b, float ln_eps, void* stream) {
    SKIMI_CHECK_ARG(in && out, "skimi_resize_bilinear: null map");
    SKIMI_CHECK_ARG(N > 0 && h > 0 && w > 0 && H > 0 && W > 0 && C > 0, "skimi_resize_bilinear: sizes must be positive");
    SKIMI_CHECK_ARG(is_elem_dtype(dtype) && (out_dtype < 0 || is_elem_dtype(out_dtype)), "skimi_resize_bilinear: bad dtype");
    SKIMI_CHECK_ARG(al16(in) && al16(out) && al16(tabx) && al16(taby), "skimi_resize_bilinear: 16-byte aligned buffers");
    return bilinear_ac_launch(in, out, dtype, N, h, w, H, W, C, (hipStream_t)stream, tabx, taby, out_dtype, ln_g, ln_b, ln_eps);
}

int skimi_resize_bilinear_planes(const float* in, void* out, int32_t N, int32_t h, int32_t w, int32_t H, int32_t W,
                                 int32_t C, const float* tabx, const float* taby, int32_t slice_records, void* zpage,
                                 void* stream) {
    SKIMI_CHECK_ARG(in && out, "skimi_resize_bilinear_planes: null map");
    SKIMI_CHECK_ARG(N > 0 && h > 0 && w > 0 && H > 0 && W > 0 && C > 0, "skimi_resize_bilinear_planes: sizes must be positive");
    SKIMI_CHECK_ARG(al16(in) && al16(out) && al16(tabx) && al16(taby) && al16(zpage),
                    "skimi_resize_bilinear_planes: 16-byte aligned buffers");
    return bilinear_ac_planes_launch(in, (unsigned short*)out, N, h, w, H, W, C, (hipStream_t)stream, tabx, taby, slice_records,
                                     zpage);
}

int skimi_add_uv_pos(void* x, int32_t dtype, const float* tabx, const float* taby, int32_t N, int32_t H, int32_t W,
                     int32_t C, void* stream) {
    SKIMI_CHECK_ARG(x && tabx && taby, "skimi_add_uv_pos: null map or table");
    SKIMI_CHECK_ARG(N > 0 && H > 0 && W > 0 && C > 0, "skimi_add_uv_pos: sizes must be positive");
    SKIMI_CHECK_ARG(is_elem_dtype(dtype), "skimi_add_uv_pos: bad dtype %d", dtype);
    SKIMI_CHECK_ARG(al16(x) && al16(tabx) && al16(taby), "skimi_add_uv_pos: 16-byte aligned buffers");
    return add_uv_pos_launch(x, dtype, tabx, taby, N, H, W, C, (hipStream_t)stream);
}

int skimi_add_uv_pos_records(const float* x, const float* tabx, const float* taby, int32_t N, int32_t H, int32_t W,
                             int32_t C, void* rec, void* stream) {
    SKIMI_CHECK_ARG(x && rec, "skimi_add_uv_pos_records: null map or records");
    SKIMI_CHECK_ARG(tabx == nullptr || taby != nullptr, "skimi_add_uv_pos_records: needs both tables or none");
    SKIMI_CHECK_ARG(N > 0 && H > 0 && W > 0 && C > 0, "skimi_add_uv_pos_records: sizes must be positive");
    SKIMI_CHECK_ARG(al16(x) && al16(tabx) && al16(taby) && al16(rec), "skimi_add_uv_pos_records: 16-byte aligned buffers");
    return add_uv_pos_records_launch(x, tabx, taby, N, H, W, C, rec, (hipStream_t)stream);
}

int skimi_dpt_out(const void* in, int32_t dtype, const float* W, const float* b, int32_t n_out, float* pts, float* conf,
                  int64_t npix, int32_t mode, void* stream) {
    SKIMI_CHECK_ARG(in && W && b && pts && conf, "skimi_dpt_out: null buffer");
    SKIMI_CHECK_ARG(npix > 0, "skimi_dpt_out: npix must be positive");
    SKIMI_CHECK_ARG(is_elem_dtype(dtype) && (mode == 0 || mode == 1), "skimi_dpt_out: bad dtype or mode");
    SKIMI_CHECK_ARG(al16(in), "skimi_dpt_out: 16-byte aligned input");
    return dpt_out_launch(in, dtype, W, b, n_out, pts, conf, (long)npix, mode, (hipStream_t)stream);
}

int skimi_patch_gather(const float* img, void* out, int32_t out_dtype, int32_t F, int32_t H, int32_t W, int32_t p,
                       int32_t Kp, void* stream) {
    SKIMI_CHECK_ARG(img && out, "skimi_patch_gather: null buffer");
    SKIMI_CHECK_ARG(F > 0 && p > 0 && H >= p && W >= p, "skimi_patch_gather: needs F > 0 and 0 < p <= H, W");
    SKIMI_CHECK_ARG(is_elem_dtype(out_dtype), "skimi_patch_gather: bad out_dtype %d", out_dtype);
    SKIMI_CHECK_ARG((long)Kp >= 3L * p * p, "skimi_patch_gather: Kp = %d is less than 3 p^2", Kp);
    return patch_gather_launch(img, out, out_dtype, F, H, W, p, Kp, (hipStream_t)stream);
}

int skimi_adaln(const float* xn, const float* x, const float* mod, float* out, int64_t rows, int32_t D, void* stream) {
    SKIMI_CHECK_ARG(xn && x && mod && out, "skimi_adaln: null buffer");
    SKIMI_CHECK_ARG(rows > 0 && D > 0, "skimi_adaln: sizes must be positive");
    return adaln_launch(xn, x, mod, out, (long)rows, D, (hipStream_t)stream);
}

int skimi_pose_update(const float* delta, float* pred_pad, float* act_out, int64_t rows, int32_t first, void* stream) {
    SKIMI_CHECK_ARG(delta && pred_pad && act_out, "skimi_pose_update: null buffer");
    SKIMI_CHECK_ARG(rows > 0, "skimi_pose_update: rows must be positive");
    return pose_update_launch(delta, pred_pad, act_out, (long)rows, first, (hipStream_t)stream);
}

int skimi_special_tokens(float* x, const float* table, int32_t F, int32_t S, int32_t P, int32_t n, int32_t C, void* stream) {
    SKIMI_CHECK_ARG(x && table, "skimi_special_tokens: null buffer");
    SKIMI_CHECK_ARG(F > 0 && S > 0 && n > 0 && C > 0, "skimi_special_tokens: sizes must be positive");
    SKIMI_CHECK_ARG(n <= P, "skimi_special_tokens: n = %d special tokens exceed the %d tokens of a frame", n, P);
    return special_tokens_launch(x, table, F, S, P, n, C, (hipStream_t)stream);
}

int skimi_track_avgpool2(const float* in, float* out, int32_t N, int32_t H, int32_t W, int32_t C, void* stream) {
    SKIMI_CHECK_ARG(in && out, "skimi_track_avgpool2: null buffer");
    SKIMI_CHECK_ARG(N > 0 && H >= 2 && W >= 2 && C > 0, "skimi_track_avgpool2: needs N, C > 0 and H, W >= 2");
    return avgpool2_launch(in, out, N, H, W, C, (hipStream_t)stream);
}

int skimi_track_sample_border(const float* fmap, int64_t img_stride, const float* coords, int64_t coord_stride, float* out,
                              int32_t B, int32_t N, int32_t H, int32_t W, int32_t C, void* stream) {
    SKIMI_CHECK_ARG(fmap && coords && out, "skimi_track_sample_border: null buffer");
    SKIMI_CHECK_ARG(B > 0 && N > 0 && H > 0 && W > 0 && C > 0, "skimi_track_sample_border: sizes must be positive");
    SKIMI_CHECK_ARG(img_stride >= (int64_t)H * W * C, "skimi_track_sample_border: img_stride is less than H * W * C");
    SKIMI_CHECK_ARG(coord_stride >= 2, "skimi_track_sample_border: coord_stride must be >= 2");
    return sample_border_launch(fmap, (long)img_stride, coords, (long)coord_stride, out, B, N, H, W, C, (hipStream_t)stream);
}

int skimi_track_corr_sample(const float* tgt, const float* fmap, const float* coords, float* out, int64_t rows, int32_t N,
                            int32_t S, int32_t H, int32_t W, int32_t C, int32_t r, int32_t level, int64_t ldo,
                            int32_t out_off, void* stream) {
    SKIMI_CHECK_ARG(tgt && fmap && coords && out, "skimi_track_corr_sample: null buffer");
    SKIMI_CHECK_ARG(rows > 0 && N > 0 && S > 0 && H > 0 && W > 0 && C > 0, "skimi_track_corr_sample: sizes must be positive");
    SKIMI_CHECK_ARG(rows % ((int64_t)N * S) == 0, "skimi_track_corr_sample: rows must be a multiple of N * S");
    SKIMI_CHECK_ARG(r >= 0 && r <= 64 && level >= 0 && level < 16, "skimi_track_corr_sample: needs 0 <= r <= 64, 0 <= level < 16");
    SKIMI_CHECK_ARG(out_off >= 0 && ldo >= (int64_t)out_off + (2 * r + 1) * (2 * r + 1),
                    "skimi_track_corr_sample: ldo is less than out_off + (2r+1)^2");
    return corr_sample_launch(tgt, fmap, coords, out, (long)rows, N, S, H, W, C, r, level, (long)ldo, out_off, (hipStream_t)stream);
}

int skimi_track_pos_embed_sample(const float* coords, int64_t coord_stride, float* out, int32_t BN, int32_t H, int32_t W,
                                 int32_t D, void* stream) {
    SKIMI_CHECK_ARG(coords && out, "skimi_track_pos_embed_sample: null buffer");
    SKIMI_CHECK_ARG(BN > 0 && H > 0 && W > 0 && D > 0, "skimi_track_pos_embed_sample: sizes must be positive");
    SKIMI_CHECK_ARG(D % 4 == 0, "skimi_track_pos_embed_sample: needs D %% 4 == 0 (got %d)", D);
    SKIMI_CHECK_ARG(coord_stride >= 2, "skimi_track_pos_embed_sample: coord_stride must be >= 2");
    return pos_embed_sample_launch(coords, (long)coord_stride, out, BN, H, W, D, (hipStream_t)stream);
}

int skimi_track_input(const float* coords, const float* fcorr, const float* tfeat, const float* pos, const float* qrt,
                      float* x, int64_t rows, int32_t S, int32_t L, int64_t ldx, float max_scale, void* stream) {
    SKIMI_CHECK_ARG(coords && fcorr && tfeat && pos && qrt && x, "skimi_track_input: null buffer");
    SKIMI_CHECK_ARG(rows > 0 && S > 0 && L > 0 && rows % S == 0, "skimi_track_input: needs rows, S, L > 0 and rows %% S == 0");
    SKIMI_CHECK_ARG(L % 4 == 0, "skimi_track_input: needs L %% 4 == 0 (got %d)", L);
    SKIMI_CHECK_ARG(ldx >= 3L * L + 4, "skimi_track_input: ldx is less than 3 L + 4");
    SKIMI_CHECK_ARG(max_scale > 0.f, "skimi_track_input: max_scale must be positive");
    return track_input_launch(coords, fcorr, tfeat, pos, qrt, x, (long)rows, S, L, (long)ldx, max_scale, (hipStream_t)stream);
}

int skimi_track_coord_update(float* coords, const float* delta, int64_t ldd, const float* query, float* pred, int64_t rows,
                             int32_t N, int32_t S, float stride, void* stream) {
    SKIMI_CHECK_ARG(coords && delta && query, "skimi_track_coord_update: null buffer");
    SKIMI_CHECK_ARG(rows > 0 && N > 0 && S > 0 && rows % ((int64_t)N * S) == 0,
                    "skimi_track_coord_update: needs rows, N, S > 0 and rows a multiple of N * S");
    SKIMI_CHECK_ARG(ldd >= 2, "skimi_track_coord_update: ldd must be >= 2");
    return track_coord_update_launch(coords, delta, (long)ldd, query, pred, (long)rows, N, S, stride, (hipStream_t)stream);
}

int skimi_track_init(const float* q, float* coords, float* qs, int64_t BN, int32_t S, float stride, void* stream) {
    SKIMI_CHECK_ARG(q && coords && qs, "skimi_track_init: null buffer");
    SKIMI_CHECK_ARG(BN > 0 && S > 0, "skimi_track_init: sizes must be positive");
    SKIMI_CHECK_ARG(stride > 0.f, "skimi_track_init: stride must be positive");
    return track_init_launch(q, coords, qs, (long)BN, S, stride, (hipStream_t)stream);
}

int skimi_track_repeat_rows(const float* src, float* dst, int64_t BN, int32_t S, int32_t C, void* stream) {
    SKIMI_CHECK_ARG(src && dst, "skimi_track_repeat_rows: null buffer");
    SKIMI_CHECK_ARG(BN > 0 && S > 0 && C > 0, "skimi_track_repeat_rows: sizes must be positive");
    return repeat_rows_launch(src, dst, (long)BN, S, C, (hipStream_t)stream);
}

int skimi_track_bns_to_bsn(const float* in, float* out, int32_t B, int32_t N, int32_t S, void* stream) {
    SKIMI_CHECK_ARG(in && out, "skimi_track_bns_to_bsn: null buffer");
    SKIMI_CHECK_ARG(B > 0 && N > 0 && S > 0, "skimi_track_bns_to_bsn: sizes must be positive");
    return bns_to_bsn_launch(in, out, B, N, S, (hipStream_t)stream);
}

}  // extern "C"
