// The forward context's launch helpers and one pre-LN transformer block of the VGGT forward
// (vggt/vggt/layers/block.py:77-98 + attention.py:50-72): the DINOv2 blocks, the aggregator's frame / global
// blocks and the camera head's trunk all run through run_block.
#include <math.h>
#include <string.h>

#include "gemm_epilogue.h"
#include "kernels.h"
#include "vggt_model.h"

namespace skimi {
namespace vggt {

void Ctx::gemm(skimi_gemm_desc& d) {
    // wide fp32-accurate 3x3 convs: lend arena scratch for the activation planes of the
    // LDS-DMA bf16x3 kernel (released right after the launch is enqueued: stream order keeps
    // later users of that memory behind it)
    const size_t mk = ar.mark();
    if (d.W_split != nullptr && d.a_dtype != SKIMI_BF16X3_REC) {
        d.x3_scratch_bytes = gemm_x3dma_scratch_bytes(&d);
        d.x3_scratch = ar.alloc(d.x3_scratch_bytes);
    }
    run([&] { return gemm_dispatch(&d, st, slab, slab_bytes, 0); });
    ar.release(mk);
}
skimi_gemm_desc Ctx::desc(const Lin& L, const void* A, int a_dt, long lda, int M, void* out, int out_dt, long ldo) {
    skimi_gemm_desc d;
    memset(&d, 0, sizeof d);
    d.M = M; d.N = L.N; d.K = L.K;
    d.A = A; d.a_dtype = a_dt; d.lda = lda;
    d.W = L.w; d.w_dtype = L.wdt; d.ldw = L.K;
    d.prec = L.prec;
    d.splitk_scratch_zeroed = 1;
    d.W_split = L.w_split;   // gemm_x3dma_eligible decides (shape, tile count)
    d.bias = L.b;
    d.out = out; d.out_dtype = out_dt; d.ldo = ldo;
    return d;
}
void Ctx::conv_geom(skimi_gemm_desc& d, const ConvW& c, int N, int H, int W, int OH, int OW) {
    if (c.k == 1 && c.stride == 1) return;   // plain rows
    d.a_mode = c.kmode;
    d.cN = N; d.cH = H; d.cW = W; d.cC = c.cin; d.KH = c.k; d.KW = c.k;
    d.stride = c.stride; d.pad = c.pad; d.dil = 1; d.OH = OH; d.OW = OW;
}
void Ctx::ln(const float* x, const float* x2, long ldx, long rows, int C, const LNw& w, float eps, void* out, int odt,
             long grp_rows, long grp_stride, long grp_off) {
    run([&] { return layernorm_launch(x, x2, ldx, rows, C, w.g, w.b, eps, out, odt, C, st, grp_rows, grp_stride, grp_off); });
}
void Ctx::copy(void* dst, const void* src, size_t bytes) {
    run([&] {
        if (hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st) == hipSuccess) return (int)SKIMI_OK;
        set_error("hipMemcpyAsync failed");
        return (int)SKIMI_ERR_HIP;
    });
}
void Ctx::zero(void* dst, size_t bytes) {
    run([&] { return hipMemsetAsync(dst, 0, bytes, st) == hipSuccess ? (int)SKIMI_OK : (int)SKIMI_ERR_HIP; });
}

// one pre-LN transformer block on the fp32 residual stream x [batch*seq, C]
// (vggt/vggt/layers/block.py:77-98 + attention.py:50-72), scratch buffers supplied by the caller
void run_block(Ctx& c, const BlockW& w, float* x, int batch, int seq, int C, int heads, float eps, bool rope,
               const BlockBufs& b) {
    const int M = batch * seq;
    const int prec = w.qkv.prec;
    const int adt = Ctx::act_dt(prec);
    // the packed q / k / v buffer: SKIMI_PREC_F16 keeps the attention products on bf16 operands (they average their rounding
    // noise over all keys: profiles/r03_precision_ablation.md), so qkv's epilogue writes bf16 and the attention kernel
    // converts its output to fp16 for proj
    const int qdt = adt == SKIMI_F16 ? SKIMI_BF16 : adt;
    const int hidden = w.fc1.N;
    const bool fp8 = w.qkv.wq != nullptr && b.q8 != nullptr;   // SKIMI_PREC_FP8: qkv, proj, fc1, fc2 on the MXFP8 MFMA
    // the quantisation rides in the producers where the shapes allow: LayerNorm writes MXFP8 directly (C % 256 == 0),
    // the attention kernel writes its output rows as MXFP8 (64-wide heads), and fc1's GELU epilogue writes the hidden
    // activation as MXFP8 (large launches on the single-stream loop)
    const bool ln_mx = fp8 && C % 256 == 0;
    const bool hid_mx = fp8 && gemm_fp8_mx_output_ok(M, hidden);
    const bool ao_mx = fp8 && w.proj.wq != nullptr && attention_mx_output_ok(qdt, heads, C / heads);
    // fp32-accurate mode: a Linear whose launch takes the LDS-DMA bf16x3 kernel reads its A operand as [hi 32 | lo 32]
    // records; where the producer can write them (LayerNorm, fc1's GELU epilogue) the fp32 copy and the split pass go
    const bool x3 = adt == SKIMI_F32 && C % 256 == 0;
    auto d_qkv = c.desc(w.qkv, b.xn, adt, C, M, b.qkv, qdt, 3 * C);
    bool rec_qkv = false;
    if (x3) {
        const auto q = Ctx::as_records(d_qkv, b.xn, (size_t)M * C * 4);
        if ((rec_qkv = gemm_x3dma_eligible(&q))) d_qkv = q;
    }
    if (ln_mx) {
        c.run([&] { return layernorm_mx_launch(x, C, M, C, w.n1.g, w.n1.b, eps, b.q8, b.q8s, c.st); });
    } else {
        c.ln(x, nullptr, C, M, C, w.n1, eps, b.xn, rec_qkv ? SKIMI_BF16X3_REC : adt);
    }
    if (fp8) {
        if (!ln_mx) c.run([&] { return quant_mx_launch(b.xn, SKIMI_BF16, C, M, C, b.q8, b.q8s, c.st); });
        c.run([&] {
            return gemm_fp8_launch(b.q8, b.q8s, w.qkv.wq, w.qkv.wq_scales, M, 3 * C, C, w.qkv.b, SKIMI_ACT_NONE, nullptr, nullptr, 0,
                                   b.qkv, SKIMI_BF16, 3 * C, c.st);
        });
    } else {
        c.gemm(d_qkv);
    }
    int q_scaled = 0;
    if (w.qn_w || rope)
        c.run([&] {
            // bf16 mode: the softmax scale (x log2 e) rides in q's one rounding to bf16, the attention kernel then
            // exponentiates the raw accumulator
            const float q_scale = (1.0f / sqrtf((float)(C / heads))) * 1.44269504088896340736f;
            return qknorm_rope_launch(b.qkv, qdt, M, heads, w.qn_w, w.qn_b, w.kn_w, w.kn_b, 1e-5f, rope ? c.tabs->pos : nullptr,
                                      c.tabs->rope_cos, c.tabs->rope_sin, c.tabs->rope_npos, c.st, q_scale,
                                      qdt == SKIMI_BF16 && C / heads == 64 ? &q_scaled : nullptr);
        });
    // fp32-accurate mode: the MLP's hidden buffer (M x hidden fp32, idle until fc1) lends the hi / lo planes of k and v; the
    // attention kernel writes proj's operand records when proj runs on the LDS-DMA kernel
    auto d_proj = c.desc(w.proj, b.ao, adt, C, M, x, SKIMI_F32, C);
    d_proj.gamma = w.ls1; d_proj.resid = x; d_proj.ldr = C;
    int ao_rec = 0;
    if (x3 && C / heads == 64) {
        const auto q = Ctx::as_records(d_proj, b.ao, (size_t)M * C * 4);
        ao_rec = gemm_x3dma_eligible(&q) ? 1 : 0;
    }
    AttnRequest req = {};
    req.qkv = b.qkv; req.out = b.ao; req.dtype = qdt; req.out_dtype = adt == SKIMI_F16 ? SKIMI_F16 : qdt;
    req.batch = batch; req.seq = seq; req.heads = heads; req.head_dim = C / heads; req.q_prescaled = q_scaled;
    if (adt == SKIMI_F32) {
        req.x3_scratch = b.hid;
        req.x3_scratch_bytes = (size_t)M * hidden * 4;
        req.want_records = ao_rec != 0;
    }
    if (ao_mx) {   // proj's MXFP8 operand: payload and scales are two buffers
        req.out = b.q8; req.out_scales = b.q8s; req.out_dtype = SKIMI_FP8MX;
    }
    c.run([&] { return attention_launch(req, c.st, &ao_rec); });
    if (ao_rec && !c.dry()) d_proj = Ctx::as_records(d_proj, b.ao, (size_t)M * C * 4);
    if (fp8 && w.proj.wq) {
        if (!ao_mx) c.run([&] { return quant_mx_launch(b.ao, SKIMI_BF16, C, M, C, b.q8, b.q8s, c.st); });
        c.run([&] {
            return gemm_fp8_launch(b.q8, b.q8s, w.proj.wq, w.proj.wq_scales, M, C, C, w.proj.b, SKIMI_ACT_NONE, w.ls1, x, C, x,
                                   SKIMI_F32, C, c.st);
        });
    } else {
        c.gemm(d_proj);
    }
    auto d_fc1 = c.desc(w.fc1, b.xn, adt, C, M, b.hid, adt, hidden);
    d_fc1.act = SKIMI_ACT_GELU;
    auto d_fc2 = c.desc(w.fc2, b.hid, adt, hidden, M, x, SKIMI_F32, C);
    d_fc2.gamma = w.ls2; d_fc2.resid = x; d_fc2.ldr = C;
    bool rec_fc1 = false;
    if (x3) {
        const auto q1 = Ctx::as_records(d_fc1, b.xn, (size_t)M * C * 4);
        if ((rec_fc1 = gemm_x3dma_eligible(&q1))) d_fc1 = q1;
        const auto q2 = Ctx::as_records(d_fc2, b.hid, (size_t)M * hidden * 4);
        if (hidden % 32 == 0 && gemm_x3dma_eligible(&q2)) {   // fc1 writes the hidden activation as fc2's records, and only so
            d_fc2 = q2;
            d_fc1.out = nullptr;
            d_fc1.out_records = b.hid;
        }
    }
    if (ln_mx) {
        c.run([&] { return layernorm_mx_launch(x, C, M, C, w.n2.g, w.n2.b, eps, b.q8, b.q8s, c.st); });
    } else {
        c.ln(x, nullptr, C, M, C, w.n2, eps, b.xn, rec_fc1 ? SKIMI_BF16X3_REC : adt);
    }
    if (fp8) {
        if (!ln_mx) c.run([&] { return quant_mx_launch(b.xn, SKIMI_BF16, C, M, C, b.q8, b.q8s, c.st); });
        // b.hid (M x hidden bf16 = 2 bytes per element) holds the MXFP8 hidden activation: payload M x hidden bytes,
        // then its scales
        unsigned char* hq = (unsigned char*)b.hid;
        unsigned char* hs = hq + (size_t)M * hidden;
        if (hid_mx) {
            c.run([&] {
                return gemm_fp8_launch(b.q8, b.q8s, w.fc1.wq, w.fc1.wq_scales, M, hidden, C, w.fc1.b, SKIMI_ACT_GELU, nullptr, nullptr, 0,
                                       hq, SKIMI_FP8MX, hidden, c.st, hs);
            });
        } else {
            c.run([&] {
                return gemm_fp8_launch(b.q8, b.q8s, w.fc1.wq, w.fc1.wq_scales, M, hidden, C, w.fc1.b, SKIMI_ACT_GELU, nullptr, nullptr, 0,
                                       b.hid, SKIMI_BF16, hidden, c.st);
            });
            c.run([&] { return quant_mx_launch(b.hid, SKIMI_BF16, hidden, M, hidden, b.q8, b.q8s, c.st); });
            hq = (unsigned char*)b.q8;
            hs = (unsigned char*)b.q8s;
        }
        c.run([&] {
            return gemm_fp8_launch(hq, hs, w.fc2.wq, w.fc2.wq_scales, M, C, hidden, w.fc2.b, SKIMI_ACT_NONE, w.ls2, x, C, x,
                                   SKIMI_F32, C, c.st);
        });
        return;
    }
    c.gemm(d_fc1);
    c.gemm(d_fc2);
}

}  // namespace vggt
}  // namespace skimi
