// DPT head of the VGGT forward (vggt/vggt/heads/dpt_head.py:172-291, its fusion blocks :366-456): depth, world
// points, and the track head's feature extractor, on the kept [frame | global] intermediates.
#include "env.h"
#include "gemm_epilogue.h"
#include "kernels.h"
#include "vggt_kernels.h"
#include "vggt_model.h"

namespace skimi {
namespace vggt {

const UvTab* find_uv(const ShapeTabs* h, int w, int hh, int C) {
    if (!h) return nullptr;
    for (const auto& t : h->uv)
        if (t.w == w && t.h == hh && t.C == C) return &t;
    return nullptr;
}

// whether a feature_only head's last upsample also applies the consumer's LayerNorm (SKIMI_TRACK_LN_FUSED=0: separate pass)
bool dpt_fused_ln(const DptW& w, int f2, int udt) {
    const bool off = !(int)env_once("SKIMI_TRACK_LN_FUSED", 1);
    return !off && w.feature_only && w.out_ln != nullptr && w.out_ln->g != nullptr && w.out_ln->b != nullptr && f2 == 128 && udt == SKIMI_F32;
}

static thread_local int tl_oc1_coarse = 0;
int dpt_oc1_coarse_count() { return tl_oc1_coarse; }

static int uv_missing() {
    set_error("uv table missing");
    return SKIMI_ERR_STATE;
}

// DPT head (vggt/vggt/heads/dpt_head.py:172-291) on the kept intermediates.
// Returns the NHWC feature map pointer for feature_only heads; otherwise writes pts / conf.
void* run_dpt(Ctx& c, const DptW& w, float* const* sf, float* const* sg, int F, int P, int nsp, int ph, int pw, int C,
              int H, int W, float* pts, float* conf, int act_mode) {
    const int prec = w.proj[0].prec;
    const int adt = Ctx::act_dt(prec);
    const size_t es = Ctx::esz(adt);
    const int D = 2 * C, np = ph * pw, feat = w.features;
    const size_t mk = c.ar.mark();
    // resized pyramid sizes
    int hh[4] = {ph * 4, ph * 2, ph, (ph - 1) / 2 + 1};
    int ww[4] = {pw * 4, pw * 2, pw, (pw - 1) / 2 + 1};
    void* rn[4];
    for (int i = 0; i < 4; ++i) rn[i] = c.ar.alloc((size_t)F * hh[i] * ww[i] * feat * es);
    // Levels whose feat -> feat convs run on the LDS-DMA bf16x3 kernel hand their activations over as
    // operand records ([feat/32][hi 32 | lo 32] per pixel, + zero page) written by the producing
    // epilogue: no split pass, and no fp32 copy at all where the only reader is the next conv.
    char* const fake = (char*)(uintptr_t)0x10000000;   // the eligibility probes' buffer: they look at alignment and distances only
    auto rec_bytes = [&](int lvl) { return (size_t)F * hh[lvl] * ww[lvl] * feat * 4 + 256; };
    auto takes_records = [&](const Lin& L, const ConvW* cw, int lvl) {
        if (adt != SKIMI_F32 || feat % 32 != 0 || L.w_split == nullptr) return false;
        auto d = Ctx::as_records(c.desc(L, nullptr, adt, feat, F * hh[lvl] * ww[lvl], fake, adt, L.N), fake, rec_bytes(lvl) - 256);
        if (cw) c.conv_geom(d, *cw, F, hh[lvl], ww[lvl], hh[lvl], ww[lvl]);
        return gemm_x3dma_eligible(&d);
    };
    bool use_rec[4];
    char* rn_rec[4] = {nullptr, nullptr, nullptr, nullptr};
    for (int i = 0; i < 4; ++i) {
        use_rec[i] = takes_records(w.ref[i].r2c1.lin, &w.ref[i].r2c1, i);
        if (use_rec[i]) rn_rec[i] = (char*)c.ar.alloc(rec_bytes(i));
    }
    {
        const size_t mk2 = c.ar.mark();
        void* lnb = c.ar.alloc((size_t)F * np * D * es);
        void* lnb_rec = adt == SKIMI_F32 ? c.ar.alloc((size_t)F * np * D * 4 + 256) : nullptr;   // LayerNorm output as bf16x3 records
        for (int i = 0; i < 4; ++i) {
            const size_t mk3 = c.ar.mark();
            void* t0 = c.ar.alloc((size_t)F * np * w.oc[i] * es);
            {
                // wide projections run on the LDS-DMA bf16x3 kernel: the LayerNorm writes their operand records
                auto d = c.desc(w.proj[i], lnb, adt, D, F * np, t0, adt, w.oc[i]);
                bool rec_in = false;
                if (adt == SKIMI_F32 && layernorm_records_ok(D) && w.proj[i].w_split != nullptr) {
                    const auto q = Ctx::as_records(d, lnb_rec, (size_t)F * np * D * 4);
                    if ((rec_in = gemm_x3dma_eligible(&q))) d = q;
                }
                c.ln(sf[i], sg[i], C, (long)F * np, D, w.norm, 1e-5f, rec_in ? lnb_rec : lnb, rec_in ? SKIMI_BF16X3_REC : adt, np, P, nsp);
                c.gemm(d);
            }
            // Levels 0 / 1: resize_layers[i] (ConvTranspose, k = stride = s) and layer{i+1}_rn (3x3) are adjacent linear
            // maps; where the folded weights exist and the launch fills the 256-row kernel they run as ONE launch of
            // s x s phase convs on the coarse map (gemm_x3w4_kernel<3>): the s^2 x larger intermediate is never written.
            // Its A operand is t0 + UV embedding as records, written by the embedding pass instead of back to t0.
            if (i < 2 && adt == SKIMI_F32 && w.fold[i].w_split != nullptr) {
                const size_t t0_bytes = (size_t)F * np * w.oc[i] * 4;
                auto d = Ctx::as_records(c.desc(w.fold[i], nullptr, adt, w.oc[i], F * np, fake, adt, feat), fake, t0_bytes);
                d.a_mode = 3; d.store_mode = 2; d.ps_s = i == 0 ? 4 : 2; d.ps_C = feat;
                d.cN = F; d.cH = ph; d.cW = pw; d.cC = w.oc[i];
                d.act = SKIMI_ACT_RELU;
                if (gemm_x3dma_eligible(&d)) {
                    char* t0_rec = (char*)c.ar.alloc(t0_bytes + 256);
                    const UvTab* t = w.pos_embed ? find_uv(c.tabs, pw, ph, w.oc[i]) : nullptr;
                    if (w.pos_embed && !t) c.run(uv_missing);
                    c.run([&] {
                        return add_uv_pos_records_launch((const float*)t0, t ? t->tx : nullptr, t ? t->ty : nullptr, F, ph, pw, w.oc[i],
                                                         t0_rec, c.st);
                    });
                    d = Ctx::as_records(d, t0_rec, t0_bytes);
                    d.out = rn[i];
                    d.out_records = rn_rec[i];
                    c.gemm(d);
                    c.ar.release(mk3);
                    continue;
                }
            }
            if (w.pos_embed)
                c.run([&] {
                    const UvTab* t = find_uv(c.tabs, pw, ph, w.oc[i]);
                    return t ? add_uv_pos_launch(t0, adt, t->tx, t->ty, F, ph, pw, w.oc[i], c.st) : uv_missing();
                });
            void* t1 = t0;
            if (i == 0 || i == 1) {
                const int s = i == 0 ? 4 : 2;
                const Lin& L = i == 0 ? w.rs0 : w.rs1;
                t1 = c.ar.alloc((size_t)F * hh[i] * ww[i] * w.oc[i] * es);
                auto d = c.desc(L, t0, adt, w.oc[i], F * np, t1, adt, w.oc[i]);
                d.store_mode = 1; d.ps_s = s; d.ps_C = w.oc[i];
                d.cN = F; d.cH = ph; d.cW = pw;
                c.gemm(d);
            } else if (i == 3) {
                t1 = c.ar.alloc((size_t)F * hh[i] * ww[i] * w.oc[i] * es);
                auto d = c.desc(w.rs3.lin, t0, adt, w.oc[i], F * hh[i] * ww[i], t1, adt, w.oc[i]);
                c.conv_geom(d, w.rs3, F, ph, pw, hh[i], ww[i]);
                c.gemm(d);
            }
            // layerN_rn: 3x3, no bias; its only consumer is a ResidualConvUnit whose in-place ReLU
            // rewrites it (dpt_head.py:376), so the ReLU is applied here once
            {
                auto d = c.desc(w.rn[i].lin, t1, adt, w.oc[i], F * hh[i] * ww[i], rn[i], adt, feat);
                c.conv_geom(d, w.rn[i], F, hh[i], ww[i], hh[i], ww[i]);
                d.act = SKIMI_ACT_RELU;
                d.out_records = rn_rec[i];
                c.gemm(d);
            }
            c.ar.release(mk3);
        }
        c.ar.release(mk2);
    }
    // RefineNet fusion 4 -> 1 (dpt_head.py:261-291, 427-456)
    void* prev = nullptr;   // previous refinenet output at this level's resolution
    char* prev_rec = nullptr;   // ... or, after the last level, the same map as bf16x3 operand records
    void* c1_coarse = nullptr;  // ... or output_conv1's result already, its taps contracted on the last level's coarse map
    for (int r = 3; r >= 0; --r) {
        const FusionW& f = w.ref[r];
        const int h0 = hh[r], w0 = ww[r];
        const int M = F * h0 * w0;
        const size_t bytes = (size_t)M * feat * es;
        const bool recs = use_rec[r];
        // a feat -> feat conv of this level: input as fp32 rows or as records
        auto conv_in = [&](const ConvW& cw, const void* in_f32, char* in_rec, void* out_f32, char* out_rec) {
            auto d = c.desc(cw.lin, in_f32, adt, feat, M, out_f32, adt, feat);
            c.conv_geom(d, cw, F, h0, w0, h0, w0);
            if (recs) d = Ctx::as_records(d, in_rec, rec_bytes(r) - 256);
            d.out_records = out_rec;
            return d;
        };
        void* cur;                  // relu(input of resConfUnit2)
        char* cur_rec = nullptr;
        void* tmp = recs ? nullptr : c.ar.alloc(bytes);
        char* tmp_rec = recs ? (char*)c.ar.alloc(rec_bytes(r)) : nullptr;
        if (f.has_r1) {
            // res = RCU1(layer_rn): conv2(relu(conv1(relu(x)))) + relu(x); output = prev + res;
            // RCU2's in-place ReLU then rewrites output -> store relu(prev + res) directly
            cur = c.ar.alloc(bytes);
            if (recs) cur_rec = (char*)c.ar.alloc(rec_bytes(r));
            auto d1 = conv_in(f.r1c1, rn[r], rn_rec[r], tmp, tmp_rec);
            d1.act = SKIMI_ACT_RELU;
            c.gemm(d1);
            auto d2 = conv_in(f.r1c2, tmp, tmp_rec, cur, cur_rec);
            d2.resid = rn[r]; d2.ldr = feat; d2.resid_dtype = adt;
            d2.resid2 = prev; d2.ldr2 = feat;
            d2.post_act = SKIMI_ACT_RELU;
            c.gemm(d2);
        } else {
            cur = rn[r];
            cur_rec = rn_rec[r];
        }
        // RCU2(cur): conv2(relu(conv1(cur))) + cur; its result is read by the 1x1 out_conv only
        const bool u_recs = recs && takes_records(f.out_conv, nullptr, r);
        void* u = u_recs ? nullptr : c.ar.alloc(bytes);
        char* u_rec = u_recs ? (char*)c.ar.alloc(rec_bytes(r)) : nullptr;
        {
            auto d1 = conv_in(f.r2c1, cur, cur_rec, tmp, tmp_rec);
            d1.act = SKIMI_ACT_RELU;
            c.gemm(d1);
            auto d2 = conv_in(f.r2c2, tmp, tmp_rec, u, u_rec);
            d2.resid = cur; d2.ldr = feat; d2.resid_dtype = adt;
            c.gemm(d2);
        }
        // dpt_head.py:447-455 upsamples (bilinear, align_corners) to the next level's size (x2 for
        // refinenet1) and then applies the 1x1 out_conv.  Both are linear maps over different axes
        // (space / channels) and the interpolation weights sum to 1, so they commute exactly, bias
        // included; the 1x1 conv runs here on the 4x smaller map, fp32 rounding order aside.
        const int h1 = r > 0 ? hh[r - 1] : 2 * h0, w1 = r > 0 ? ww[r - 1] : 2 * w0;
        // refinenet1's upsample is followed directly by output_conv1 (3x3, pad 1; dpt_head.py:287): that conv's channel
        // contraction commutes with the upsample tap by tap, so where the nine taps are packed as 1x1 matrices (oc1t) and
        // their GEMM fills the 256-row kernel, they are contracted HERE, on the 4x smaller map (a quarter of the MFMAs),
        // and the upsample sums the nine shifted, resized results under the conv's padding mask (dpt_tap_sum_launch).
        // out_conv hands its result over as operand records only.
        if (r == 0 && !w.feature_only && adt == SKIMI_F32 && w.oc1t.w_split != nullptr && feat % 32 == 0) {
            const size_t orec_bytes = (size_t)M * feat * 4;
            auto dt = Ctx::as_records(c.desc(w.oc1t, nullptr, adt, feat, M, fake, adt, w.oc1t.N), fake, orec_bytes);
            if (gemm_x3dma_eligible(&dt)) {   // pointer-independent up to alignment: the sizing pass agrees
                c1_coarse = c.ar.alloc((size_t)F * h1 * w1 * (feat / 2) * 4);   // outlives the taps: allocated below them
                const size_t mk_t = c.ar.mark();
                char* orec = (char*)c.ar.alloc(orec_bytes + 256);
                float* taps = (float*)c.ar.alloc((size_t)M * w.oc1t.N * 4);   // [pixel][tap][feat / 2]
                auto d = c.desc(f.out_conv, u, adt, feat, M, nullptr, adt, feat);
                if (u_recs) d = Ctx::as_records(d, u_rec, rec_bytes(r) - 256);
                d.out_records = orec;
                c.gemm(d);
                dt = Ctx::as_records(c.desc(w.oc1t, nullptr, adt, feat, M, taps, adt, w.oc1t.N), orec, orec_bytes);
                c.gemm(dt);
                c.run([&] { return dpt_tap_sum_launch(taps, w.oc1.lin.b, (float*)c1_coarse, F, h0, w0, feat / 2, c.st); });
                if (!c.dry()) ++tl_oc1_coarse;
                c.ar.release(mk_t);   // stream order keeps the tail's users of this memory behind the tap sum
                prev = nullptr;
                hh[r] = h1; ww[r] = w1;
                continue;
            }
        }
        void* olow = c.ar.alloc(bytes);
        {
            auto d = c.desc(f.out_conv, u, adt, feat, M, olow, adt, feat);
            if (u_recs) d = Ctx::as_records(d, u_rec, rec_bytes(r) - 256);
            c.gemm(d);
        }
        // The last level's upsampled map is read by output_conv1 only: when that conv runs on the
        // LDS-DMA bf16x3 kernel the upsample writes its operand records ([C/32][hi 32 | lo 32] per
        // pixel + the zero page) instead of fp32 (no fp32 round trip, no split pass).
        if (r == 0 && adt == SKIMI_F32 && w.oc1.lin.w_split != nullptr && feat % 32 == 0) {
            const size_t rec_bytes = (size_t)F * h1 * w1 * feat * 4;
            const size_t mk_rec = c.ar.mark();
            char* rec = (char*)c.ar.alloc(rec_bytes + 256);
            // out: a placeholder for the eligibility query only
            auto d = Ctx::as_records(c.desc(w.oc1.lin, nullptr, adt, feat, F * h1 * w1, rec, adt, w.feature_only ? feat : feat / 2), rec,
                                     rec_bytes);
            c.conv_geom(d, w.oc1, F, h1, w1, h1, w1);
            if (gemm_x3dma_eligible(&d)) {   // pointer-independent up to alignment: the sizing pass agrees
                prev_rec = rec;
                c.run([&] {
                    return bilinear_ac_planes_launch((const float*)olow, (unsigned short*)rec, F, h0, w0, h1, w1, feat, c.st,
                                                     nullptr, nullptr, 1, rec + rec_bytes);
                });
                prev = nullptr;
                hh[r] = h1; ww[r] = w1;
                continue;
            }
            c.ar.release(mk_rec);
        }
        void* o = c.ar.alloc((size_t)F * h1 * w1 * feat * es);
        c.run([&] { return bilinear_ac_launch(olow, o, adt, F, h0, w0, h1, w1, feat, c.st); });
        prev = o;
        hh[r] = h1; ww[r] = w1;   // resolution of `prev`
    }
    const int h1 = hh[0], w1 = ww[0];
    const int f2 = w.feature_only ? feat : feat / 2;
    void* c1 = c1_coarse ? c1_coarse : c.ar.alloc((size_t)F * h1 * w1 * f2 * es);
    if (c1_coarse != nullptr) {
        // output_conv1 has run
    } else if (prev_rec != nullptr) {
        auto d = Ctx::as_records(c.desc(w.oc1.lin, nullptr, adt, feat, F * h1 * w1, c1, adt, f2), prev_rec, (size_t)F * h1 * w1 * feat * 4);
        c.conv_geom(d, w.oc1, F, h1, w1, h1, w1);
        c.gemm(d);
    } else {
        auto d = c.desc(w.oc1.lin, prev, adt, feat, F * h1 * w1, c1, adt, f2);
        c.conv_geom(d, w.oc1, F, h1, w1, h1, w1);
        c.gemm(d);
    }
    const int Ho = ph * c.h->cfg.patch_size / w.down_ratio, Wo = pw * c.h->cfg.patch_size / w.down_ratio;
    const UvTab* uvt = w.pos_embed ? find_uv(c.tabs, Wo, Ho, f2) : nullptr;
    if (w.pos_embed && !uvt) c.run(uv_missing);
    const int no_direct = !(int)env_once("SKIMI_CONV_DIRECT", 1);   // A/B timing
    const bool direct = !w.feature_only && w.oc2a_direct != nullptr && adt == SKIMI_F32 && !no_direct;
    void* c2 = nullptr;
    if (direct) {
        // upsample (+ UV embedding) straight into bf16 hi / lo planes, then the direct 3x3 -> 32 conv
        // (shapes and a switch decide: the sizing pass agrees); where every window's source samples fit its staging,
        // the conv interpolates them itself and the records never exist
        const bool up = conv_direct_n32_up_eligible(h1, w1, Ho, Wo, f2);
        const size_t pe = (size_t)F * Ho * Wo * f2;
        unsigned short* rec = up ? nullptr : (unsigned short*)c.ar.alloc(pe * 4);   // [pixel][hi f2 | lo f2]
        c2 = c.ar.alloc((size_t)F * Ho * Wo * 32 * es);
        if (up) {
            c.run([&] {
                return conv_direct_n32_up_launch((const float*)c1, h1, w1, uvt ? uvt->tx : nullptr, uvt ? uvt->ty : nullptr,
                                                 w.oc2a_direct, w.oc2a.lin.b, (float*)c2, F, Ho, Wo, f2, 1, c.st);
            });
        } else {
            c.run([&] {
                return bilinear_ac_planes_launch((const float*)c1, rec, F, h1, w1, Ho, Wo, f2, c.st, uvt ? uvt->tx : nullptr,
                                                 uvt ? uvt->ty : nullptr);
            });
            c.run([&] {
                return conv_direct_n32_launch(rec, rec + f2, w.oc2a_direct, w.oc2a.lin.b, (float*)c2, F, Ho, Wo, f2, 1, c.st,
                                              2L * f2);
            });
        }
    } else {
        const int udt = (w.feature_only && w.out_f32) ? SKIMI_F32 : adt;   // the tracker's feature map: fp32 out of the last upsample
        void* c1u = c.ar.alloc((size_t)F * Ho * Wo * f2 * Ctx::esz(udt));
        // upsample to the output size with the UV positional embedding added in the same pass
        c.run([&] {
            return dpt_fused_ln(w, f2, udt)
                       ? bilinear_ac_launch(c1, c1u, adt, F, h1, w1, Ho, Wo, f2, c.st, uvt ? uvt->tx : nullptr, uvt ? uvt->ty : nullptr, udt,
                                            w.out_ln->g, w.out_ln->b, 1e-5f)
                       : bilinear_ac_launch(c1, c1u, adt, F, h1, w1, Ho, Wo, f2, c.st, uvt ? uvt->tx : nullptr, uvt ? uvt->ty : nullptr, udt);
        });
        if (w.feature_only) return c1u;   // caller releases the arena
        c2 = c.ar.alloc((size_t)F * Ho * Wo * 32 * es);
        auto d = c.desc(w.oc2a.lin, c1u, adt, f2, F * Ho * Wo, c2, adt, 32);
        c.conv_geom(d, w.oc2a, F, Ho, Wo, Ho, Wo);
        d.act = SKIMI_ACT_RELU;
        c.gemm(d);
    }
    c.run([&] { return dpt_out_launch(c2, adt, w.oc2b_w, w.oc2b_b, w.n_out, pts, conf, (long)F * Ho * Wo, act_mode, c.st); });
    c.ar.release(mk);
    (void)H; (void)W;
    return nullptr;
}

}  // namespace vggt
}  // namespace skimi
