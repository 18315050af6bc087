// Track head of the VGGT forward: its weight packing and its forward.
// Reference: vggt/vggt/heads/track_head.py:72-104, track_modules/base_track_predictor.py:82-209,
// track_modules/blocks.py:90-236, track_modules/modules.py:133-204.
// Token streams are kept in (b, n, s) row order (the update-former's native order): all point tokens
// [B, N, S] first, then all virtual tokens [B, V, S], so that every stage of the update-former is ONE set of
// launches for the whole batch; the space attention reads them through strides (two-level batch (b, s))
// instead of permuting them.
#include <math.h>

#include "env.h"
#include "kernels.h"
#include "track_kernels.h"
#include "vggt_model.h"

namespace skimi {
namespace vggt {

// MFMA mode of the track head's contractions.  The reference runs the track head INSIDE its bf16 autocast region
// (models/vggt.py:85-91, unlike the camera / depth / point heads of vggt.py:65): under the 16-bit aggregator modes
// (BF16, F16, FP8) its Linears and convolutions take that mode's 16-bit operands (weights packed once, fp32
// activations rounded while staged), one MFMA per product; under BF16X3 it is fp32-accurate like everything else.
static int track_prec(const skimi_vggt_config& cfg) {
    const bool force_x3 = (int)env_once("SKIMI_TRACK_X3", 0) != 0;   // A/B timing: round 2's fp32-accurate track head
    if (cfg.prec == SKIMI_PREC_BF16X3 || force_x3) return SKIMI_PREC_BF16X3;
    return cfg.prec == SKIMI_PREC_F16 ? SKIMI_PREC_F16 : SKIMI_PREC_BF16;
}

static MhaW pack_mha(Packer& pk, const std::string& p, int H, bool cross) {
    const int X3 = track_prec(pk.h->cfg);
    MhaW w;
    w.cross = cross;
    w.n1 = pk.ln(p + ".norm1", H);
    w.n2 = pk.ln(p + ".norm2", H);
    const std::string a = p + (cross ? ".cross_attn" : ".attn");
    float* ipw = pk.raw(a + ".in_proj_weight", (int64_t)3 * H * H);
    float* ipb = pk.raw(a + ".in_proj_bias", (int64_t)3 * H);
    if (pk.rc) return w;
    auto bias_slice = [&](int off, int n) -> float* {
        float* d = (float*)pk.dmalloc((size_t)n * 4);
        if (d && hipMemcpyAsync(d, ipb + off, (size_t)n * 4, hipMemcpyDeviceToDevice, pk.st) != hipSuccess) pk.rc = SKIMI_ERR_HIP;
        return d;
    };
    if (cross) {
        w.nctx = pk.ln(p + ".norm_context", H);
        w.q_proj = pk.pack_matrix(ipw, H, H, X3);
        w.q_proj.b = bias_slice(0, H);
        w.kv_proj = pk.pack_matrix(ipw + (size_t)H * H, 2 * H, H, X3);
        w.kv_proj.b = bias_slice(H, 2 * H);
    } else {
        w.in_proj = pk.pack_matrix(ipw, 3 * H, H, X3);
        w.in_proj.b = bias_slice(0, 3 * H);
    }
    w.out_proj = pk.linear(a + ".out_proj", H, H, X3);
    w.fc1 = pk.linear(p + ".mlp.fc1", 4 * H, H, X3);
    w.fc2 = pk.linear(p + ".mlp.fc2", H, 4 * H, X3);
    return w;
}

void pack_track(Packer& pk, skimi_vggt* h) {
    const skimi_vggt_config& cfg = h->cfg;
    const int X3 = track_prec(cfg);
    const int D = 2 * cfg.embed_dim, L = cfg.track_features, Hh = cfg.track_hidden, V = cfg.track_virtual;
    const int tdim = 3 * L + 4;
    const int corr_in = cfg.track_corr_levels * (2 * cfg.track_corr_radius + 1) * (2 * cfg.track_corr_radius + 1);
    // under a 16-bit mode the feature extractor's activations travel in that format (LDS-DMA GEMMs for its wide projections,
    // 16-bit gathers for its convolutions); its last upsample writes the fp32 feature map the tracker consumes
    h->trackf = pk.dpt("track_head.feature_extractor", D, L, cfg.dpt_out_channels, 4, true, X3);
    h->trackf.out_f32 = true;
    h->trackf.pos_embed = false;
    h->trackf.down_ratio = 2;
    TrackW& t = h->track;
    const std::string K = "track_head.tracker", U = K + ".updateformer";
    t.qrt = pk.keep(K + ".query_ref_token", (int64_t)2 * tdim);
    t.virt = pk.keep(U + ".virual_tracks", (int64_t)V * Hh);
    t.corr_fc1 = pk.linear(K + ".corr_mlp.fc1", Hh, corr_in, X3);
    t.corr_fc2 = pk.linear(K + ".corr_mlp.fc2", L, Hh, X3);
    t.input_norm = pk.ln(U + ".input_norm", tdim);
    t.input_transform = pk.linear(U + ".input_transform", Hh, tdim, X3);
    t.output_norm = pk.ln(U + ".output_norm", Hh);
    t.flow_head = pk.linear(U + ".flow_head", L + 2, Hh, X3);
    t.time.clear(); t.space_virtual.clear(); t.p2v.clear(); t.v2p.clear();
    for (int i = 0; i < cfg.track_depth; ++i) {
        const std::string si = std::to_string(i);
        t.time.push_back(pack_mha(pk, U + ".time_blocks." + si, Hh, false));
        t.space_virtual.push_back(pack_mha(pk, U + ".space_virtual_blocks." + si, Hh, false));
        t.p2v.push_back(pack_mha(pk, U + ".space_point2virtual_blocks." + si, Hh, true));
        t.v2p.push_back(pack_mha(pk, U + ".space_virtual2point_blocks." + si, Hh, true));
    }
    t.fmap_norm = pk.ln(K + ".fmap_norm", L);
    h->trackf.out_ln = &t.fmap_norm;   // applied by the extractor's last upsample when L == 128 (run_dpt)
    t.ffeat_norm = pk.ln(K + ".ffeat_norm", L);   // GroupNorm(1, L) on [rows, L] == LayerNorm(L)
    t.ffeat_updater = pk.linear(K + ".ffeat_updater.0", L, L, X3);
    t.vis = pk.linear(K + ".vis_predictor.0", 1, L, X3);
    t.conf = pk.linear(K + ".conf_predictor.0", 1, L, X3);
}

// One AttnBlock / CrossAttnBlock.  xq: rq contiguous rows of Hh (in/out).  The attention sees
// `outer` x `batch` sequences; token t of sequence (go, bi) sits at row
// go*q_outer_rows + bi*q_batch_rows + t*q_tok_rows  of the q stream (and likewise k_* in the context stream).
static void run_mha(Ctx& c, const MhaW& w, float* xq, long rq, const float* ctx, long rk, int batch, int seq_q, int seq_k,
                    long q_tok_rows, long q_batch_rows, long k_tok_rows, long k_batch_rows, int heads, int Hh, const MhaBufs& b,
                    const float* resid2, int outer = 1, long q_outer_rows = 0, long k_outer_rows = 0) {
    const int hd = Hh / heads;
    // x = norm1(x): the block's residual is taken from the NORMED tensor (modules.py:160-168)
    c.ln(xq, nullptr, Hh, rq, Hh, w.n1, 1e-5f, b.xn, SKIMI_F32);
    AttnArgs a;
    a.batch = batch * outer; a.heads = heads; a.seq_q = seq_q; a.seq_k = seq_k; a.head_dim = hd;
    if (outer > 1) a.batch_inner = batch;
    a.scale = 1.0f / sqrtf((float)hd);
    a.out = b.ao;
    a.o_row = q_tok_rows * Hh; a.o_batch = q_batch_rows * Hh; a.o_head = hd;
    a.o_batch2 = q_outer_rows * Hh;
    a.q_head = a.k_head = a.v_head = hd;
    if (!w.cross) {
        auto d = c.desc(w.in_proj, b.xn, SKIMI_F32, Hh, (int)rq, b.q, SKIMI_F32, 3 * Hh);
        c.gemm(d);
        a.q = b.q; a.k = b.q + Hh; a.v = b.q + 2 * Hh;
        a.q_row = a.k_row = a.v_row = q_tok_rows * 3 * Hh;
        a.q_batch = a.k_batch = a.v_batch = q_batch_rows * 3 * Hh;
        a.q_batch2 = a.k_batch2 = a.v_batch2 = q_outer_rows * 3 * Hh;
    } else {
        c.ln(ctx, nullptr, Hh, rk, Hh, w.nctx, 1e-5f, b.cn, SKIMI_F32);
        auto dq = c.desc(w.q_proj, b.xn, SKIMI_F32, Hh, (int)rq, b.q, SKIMI_F32, Hh);
        c.gemm(dq);
        auto dk = c.desc(w.kv_proj, b.cn, SKIMI_F32, Hh, (int)rk, b.kv, SKIMI_F32, 2 * Hh);
        c.gemm(dk);
        a.q = b.q; a.k = b.kv; a.v = b.kv + Hh;
        a.q_row = q_tok_rows * Hh; a.q_batch = q_batch_rows * Hh; a.q_batch2 = q_outer_rows * Hh;
        a.k_row = a.v_row = k_tok_rows * 2 * Hh; a.k_batch = a.v_batch = k_batch_rows * 2 * Hh;
        a.k_batch2 = a.v_batch2 = k_outer_rows * 2 * Hh;
    }
    c.run([&] { return attention_f32_launch(a, c.st); });
    {
        auto d = c.desc(w.out_proj, b.ao, SKIMI_F32, Hh, (int)rq, xq, SKIMI_F32, Hh);
        d.resid = b.xn; d.ldr = Hh;
        c.gemm(d);
    }
    c.ln(xq, nullptr, Hh, rq, Hh, w.n2, 1e-5f, b.xn, SKIMI_F32);
    {
        auto d = c.desc(w.fc1, b.xn, SKIMI_F32, Hh, (int)rq, b.hid, SKIMI_F32, 4 * Hh);
        d.act = SKIMI_ACT_GELU;
        c.gemm(d);
    }
    {
        auto d = c.desc(w.fc2, b.hid, SKIMI_F32, 4 * Hh, (int)rq, xq, SKIMI_F32, Hh);
        d.resid = xq; d.ldr = Hh;
        if (resid2) { d.resid2 = resid2; d.ldr2 = Hh; }
        c.gemm(d);
    }
}

void run_track(Ctx& c, float* const* sf, float* const* sg, int B, int S, int P, int nsp, int ph, int pw, int C, int H, int W,
               const float* query, int N, float* out_track, float* out_vis, float* out_conf) {
    skimi_vggt* h = c.h;
    const skimi_vggt_config& cfg = h->cfg;
    const TrackW& w = h->track;
    const int F = B * S, L = cfg.track_features, Hh = cfg.track_hidden, V = cfg.track_virtual, heads = cfg.track_heads;
    const int tdim = 3 * L + 4, ldx = (int)align_up((size_t)tdim, 8);
    const int r = cfg.track_corr_radius, ns = (2 * r + 1) * (2 * r + 1), levels = cfg.track_corr_levels;
    const int ldc = (int)align_up((size_t)levels * ns, 8);
    const float stride = 2.0f, max_scale = 518.0f;   // track_head.py:23, base_track_predictor.py:27
    const size_t mk = c.ar.mark();
    // feature maps [F, HH, WW, L] (DPT, feature_only, down_ratio 2) -> LayerNorm over channels
    float* fm = (float*)run_dpt(c, h->trackf, sf, sg, F, P, nsp, ph, pw, C, H, W, nullptr, nullptr, 0);
    const int HH = ph * cfg.patch_size / 2, WW = pw * cfg.patch_size / 2;
    std::vector<float*> pyr(levels);
    std::vector<int> lh(levels), lw(levels);
    lh[0] = HH; lw[0] = WW;
    if (dpt_fused_ln(h->trackf, L, h->trackf.out_f32 ? SKIMI_F32 : -1)) {
        pyr[0] = fm;   // the extractor's last upsample has applied fmap_norm already (bilinear_ac_kernel<.., LN>)
    } else {
        pyr[0] = (float*)c.ar.alloc((size_t)F * HH * WW * L * 4);
        c.ln(fm, nullptr, L, (long)F * HH * WW, L, w.fmap_norm, 1e-5f, pyr[0], SKIMI_F32);
    }
    for (int l = 1; l < levels; ++l) {
        lh[l] = lh[l - 1] / 2; lw[l] = lw[l - 1] / 2;
        if (lh[l] < 1 || lw[l] < 1) {
            set_error("track head: feature map %dx%d too small for %d correlation levels", HH, WW, levels);
            c.rc = SKIMI_ERR_ARG;
            return;
        }
        pyr[l] = (float*)c.ar.alloc((size_t)F * lh[l] * lw[l] * L * 4);
        c.run([&] { return avgpool2_launch(pyr[l - 1], pyr[l], F, lh[l - 1], lw[l - 1], L, c.st); });
    }
    const long BN = (long)B * N, rows = BN * S;
    float* coords = (float*)c.ar.alloc((size_t)rows * 2 * 4);
    float* qs = (float*)c.ar.alloc((size_t)BN * 2 * 4);
    float* qfeat = (float*)c.ar.alloc((size_t)BN * L * 4);
    float* tfeat = (float*)c.ar.alloc((size_t)rows * L * 4);
    float* pos = (float*)c.ar.alloc((size_t)BN * tdim * 4);
    float* fcorr = (float*)c.ar.alloc((size_t)rows * ldc * 4);
    float* ch = (float*)c.ar.alloc((size_t)rows * Hh * 4);
    float* fc = (float*)c.ar.alloc((size_t)rows * L * 4);
    float* xin = (float*)c.ar.alloc((size_t)rows * ldx * 4);
    float* xinn = (float*)c.ar.alloc((size_t)rows * ldx * 4);
    float* init = (float*)c.ar.alloc((size_t)rows * Hh * 4);
    const long R2 = (long)B * (N + V) * S;
    float* X = (float*)c.ar.alloc((size_t)R2 * Hh * 4);
    float* fin = (float*)c.ar.alloc((size_t)rows * Hh * 4);
    float* delta = (float*)c.ar.alloc((size_t)rows * (L + 2) * 4);
    float* gn = (float*)c.ar.alloc((size_t)rows * L * 4);
    float* sc = (float*)c.ar.alloc((size_t)rows * 4);
    MhaBufs mb;
    mb.xn = (float*)c.ar.alloc((size_t)R2 * Hh * 4);
    mb.cn = (float*)c.ar.alloc((size_t)R2 * Hh * 4);
    mb.q = (float*)c.ar.alloc((size_t)R2 * 3 * Hh * 4);
    mb.kv = (float*)c.ar.alloc((size_t)R2 * 2 * Hh * 4);
    mb.ao = (float*)c.ar.alloc((size_t)R2 * Hh * 4);
    mb.hid = (float*)c.ar.alloc((size_t)R2 * 4 * Hh * 4);
    c.run([&] { return track_init_launch(query, coords, qs, BN, S, stride, c.st); });
    // query features from frame 0 of every batch element (base_track_predictor.py:113-116)
    c.run([&] { return sample_border_launch(pyr[0], (long)S * HH * WW * L, qs, 2, qfeat, B, N, HH, WW, L, c.st); });
    c.run([&] { return repeat_rows_launch(qfeat, tfeat, BN, S, L, c.st); });
    c.run([&] { return pos_embed_sample_launch(qs, 2, pos, (int)BN, HH, WW, tdim, c.st); });
    c.zero(fcorr, (size_t)rows * ldc * 4);
    c.zero(xinn, (size_t)rows * ldx * 4);
    for (int it = 0; it < cfg.track_iters && !c.rc; ++it) {
        for (int l = 0; l < levels; ++l)
            c.run([&] {
                return corr_sample_launch(tfeat, pyr[l], coords, fcorr, rows, N, S, lh[l], lw[l], L, r, l, ldc, l * ns, c.st);
            });
        {
            auto d = c.desc(w.corr_fc1, fcorr, SKIMI_F32, ldc, (int)rows, ch, SKIMI_F32, Hh);
            d.act = SKIMI_ACT_GELU;
            c.gemm(d);
            auto d2 = c.desc(w.corr_fc2, ch, SKIMI_F32, Hh, (int)rows, fc, SKIMI_F32, L);
            c.gemm(d2);
        }
        c.run([&] { return track_input_launch(coords, fc, tfeat, pos, w.qrt, xin, rows, S, L, ldx, max_scale, c.st); });
        // ---- EfficientUpdateFormer (blocks.py:90-134) ----
        c.run([&] {   // not c.ln: the output rows keep the padded stride ldx
            return layernorm_launch(xin, nullptr, ldx, rows, tdim, w.input_norm.g, w.input_norm.b, 1e-5f, xinn, SKIMI_F32,
                                    ldx, c.st);
        });
        {
            auto d = c.desc(w.input_transform, xinn, SKIMI_F32, ldx, (int)rows, init, SKIMI_F32, Hh);
            c.gemm(d);
            c.copy(X, init, (size_t)rows * Hh * 4);     // the point tokens [B, N, S] open the token stream
        }
        float* Pt = X;                                  // [B, N, S, Hh]
        float* Vt = X + rows * Hh;                      // [B, V, S, Hh]
        for (int b = 0; b < B; ++b)
            c.run([&] { return repeat_rows_launch(w.virt, Vt + (long)b * V * S * Hh, V, S, Hh, c.st); });
        for (int i = 0; i < cfg.track_depth && !c.rc; ++i) {
            // time attention: every track (points + virtual) attends over its S frames
            run_mha(c, w.time[i], X, R2, nullptr, 0, B * (N + V), S, S, 1, S, 1, S, heads, Hh, mb, nullptr);
            // space attention, whole batch per launch: per (b, frame s) a sequence over tracks -> token stride S rows,
            // inner batch (s) stride 1 row, outer batch (b) stride V*S (virtual) / N*S (points) rows
            run_mha(c, w.v2p[i], Vt, (long)B * V * S, Pt, (long)B * N * S, S, V, N, S, 1, S, 1, heads, Hh, mb, nullptr, B,
                    (long)V * S, (long)N * S);
            run_mha(c, w.space_virtual[i], Vt, (long)B * V * S, nullptr, 0, S, V, V, S, 1, S, 1, heads, Hh, mb, nullptr, B,
                    (long)V * S, (long)V * S);
            // last round: fold "tokens[:, :N] + init_tokens" (blocks.py:127) into the final epilogue
            const float* r2 = (i == cfg.track_depth - 1) ? init : nullptr;
            run_mha(c, w.p2v[i], Pt, (long)B * N * S, Vt, (long)B * V * S, S, N, V, S, 1, S, 1, heads, Hh, mb, r2, B,
                    (long)N * S, (long)V * S);
        }
        // output_norm + flow_head on the point tokens (the first B*N*S rows of X)
        c.ln(X, nullptr, Hh, rows, Hh, w.output_norm, 1e-5f, fin, SKIMI_F32);
        {
            auto d = c.desc(w.flow_head, fin, SKIMI_F32, Hh, (int)rows, delta, SKIMI_F32, L + 2);
            c.gemm(d);
        }
        // track_feats = ffeat_updater(ffeat_norm(delta_feats)) + track_feats (base_track_predictor.py:176-180)
        c.ln(delta + 2, nullptr, L + 2, rows, L, w.ffeat_norm, 1e-5f, gn, SKIMI_F32);
        {
            auto d = c.desc(w.ffeat_updater, gn, SKIMI_F32, L, (int)rows, tfeat, SKIMI_F32, L);
            d.act = SKIMI_ACT_GELU;
            d.resid = tfeat; d.ldr = L;
            c.gemm(d);
        }
        float* pred = (it == cfg.track_iters - 1) ? out_track : nullptr;
        c.run([&] { return track_coord_update_launch(coords, delta, L + 2, qs, pred, rows, N, S, stride, c.st); });
    }
    // visibility / confidence: sigmoid(Linear(track_feats)) (base_track_predictor.py:196-205)
    for (int k = 0; k < 2; ++k) {
        float* dst = k == 0 ? out_vis : out_conf;
        if (!dst) continue;
        auto d = c.desc(k == 0 ? w.vis : w.conf, tfeat, SKIMI_F32, L, (int)rows, sc, SKIMI_F32, 1);
        d.act = SKIMI_ACT_SIGMOID;
        c.gemm(d);
        c.run([&] { return bns_to_bsn_launch(sc, dst, B, N, S, c.st); });
    }
    c.ar.release(mk);
}

}  // namespace vggt
}  // namespace skimi
