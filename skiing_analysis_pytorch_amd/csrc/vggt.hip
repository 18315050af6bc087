// VGGT forward on MI355X: the graph of fused MFMA contractions, flash attention and row-wise
// kernels that replaces `preds = self.vggt(imgs)` (vggt/vggt/infer.py:84).
//
// Data layout in HBM (all channels-last, row-major):
//   residual stream x      fp32 [F*P, C]          F = B*S frames, P = 1 + R + ph*pw tokens
//   GEMM operands          bf16 (PREC_BF16) or fp32 (PREC_BF16X3) [rows, C | 3C | 4C]
//   kept intermediates     fp32 [F*P, C] x {frame, global} for the 4 DPT layers + the last layer;
//                          the reference's torch.cat([frame, global], -1) (aggregator.py:250-253) is
//                          never materialised: consumers read the two halves through two pointers
//   DPT feature maps       [F, h, w, C] (NHWC), 3x3 / strided / transposed convs as implicit-gather GEMMs
// Weights are repacked once in skimi_vggt_finalize (conv taps -> [Cout, ky, kx, Cin], ConvTranspose
// -> pixel-shuffle GEMM, bf16 copies, K padded to 8).  The forward allocates nothing: every
// activation lives in the caller's workspace through a bump arena whose peak is computed by a
// dry run of the same code (skimi_vggt_workspace_bytes).
//
// This file: the per-shape tables, the forward's plan (aggregator + which heads run) and the C API.  The parts live in
// vggt_pack.hip (weights), vggt_block.hip, vggt_camera.hip, vggt_dpt.hip and vggt_track.hip; vggt_model.h is what they share.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <memory>
#include <mutex>
#include <vector>

#include "kernels.h"
#include "vggt_kernels.h"
#include "vggt_model.h"

using namespace skimi;
using namespace skimi::vggt;

// Looks up an (H, W) entry with room for F frames or builds one.  Called with h->prep_mu held.  A build that fails
// part-way publishes nothing (the half-built entry frees its device buffers on the way out).
static int prepare(skimi_vggt* h, int F, int S, int H, int W, const ShapeTabs** out) {
    auto& entries = h->tabs[std::make_pair(H, W)];
    int largest = 0;
    for (const auto& e : entries) {
        if (e->frames >= F) {
            *out = e.get();
            return SKIMI_OK;
        }
        largest = std::max(largest, e->frames);
    }
    const ShapeTabs* first = entries.empty() ? nullptr : entries.front().get();
    const int cap = std::max(F, 2 * largest);
    (void)S;
    std::unique_ptr<ShapeTabs> tabs(new ShapeTabs());
    ShapeTabs* t_ = tabs.get();
    t_->frames = cap;
    const skimi_vggt_config& cfg = h->cfg;
    const int p = cfg.patch_size, ph = H / p, pw = W / p, nsp = 1 + cfg.num_register_tokens, P = nsp + ph * pw;
    auto up = [&](const void* src, size_t bytes, void** dst) -> int {
        SKIMI_HIP(hipMalloc(dst, bytes));
        t_->owned.push_back(*dst);
        SKIMI_HIP(hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice));
        return SKIMI_OK;
    };
    int rc;
    if (cfg.use_dino) {
        const bool native = H == W && H == cfg.dino_img_size;
        t_->dino_pos = native ? h->dino_pos : h->dino_pos_alt.at({H, W});   // presence checked by check_shape
    }
    // positions: (y, x) + 1 for patches, 0 for the special tokens (rope.py:39-59, aggregator.py:219-228)
    std::vector<int> pos((size_t)cap * P * 2, 0);
    for (int f = 0; f < cap; ++f)
        for (int y = 0; y < ph; ++y)
            for (int x = 0; x < pw; ++x) {
                const size_t i = ((size_t)f * P + nsp + (size_t)y * pw + x) * 2;
                pos[i] = y + 1;
                pos[i + 1] = x + 1;
            }
    if ((rc = up(pos.data(), pos.size() * 4, (void**)&t_->pos))) return rc;
    if (first) {   // RoPE / UV tables depend on (H, W) only: shared with (and owned by) the first entry of this frame size
        t_->rope_cos = first->rope_cos; t_->rope_sin = first->rope_sin; t_->rope_npos = first->rope_npos;
        t_->uv = first->uv;
        *out = t_;
        entries.push_back(std::move(tabs));
        return SKIMI_OK;
    }
    // RoPE tables (rope.py:86-117), fp32 arithmetic as torch: 1/100^(i/16), pos*inv_freq, cos/sin
    const int npos = std::max(ph, pw) + 1;
    std::vector<float> cs((size_t)npos * 16), sn((size_t)npos * 16);
    for (int i = 0; i < 16; ++i) {
        const float expo = (float)(2 * i) / 32.0f;
        const float inv = 1.0f / powf(100.0f, expo);
        for (int q = 0; q < npos; ++q) {
            const float a = (float)q * inv;
            cs[(size_t)q * 16 + i] = cosf(a);
            sn[(size_t)q * 16 + i] = sinf(a);
        }
    }
    if ((rc = up(cs.data(), cs.size() * 4, (void**)&t_->rope_cos))) return rc;
    if ((rc = up(sn.data(), sn.size() * 4, (void**)&t_->rope_sin))) return rc;
    t_->rope_npos = npos;
    // UV sin/cos tables (heads/utils.py:11-109 via dpt_head.py:249-259), float64 then float, x 0.1
    auto add_uv = [&](int w, int hh, int C) -> int {
        if (find_uv(t_, w, hh, C)) return SKIMI_OK;
        const double aspect = (double)W / (double)H;
        const double diag = sqrt(aspect * aspect + 1.0);
        const double sx = aspect / diag, sy = 1.0 / diag;
        const int half = C / 2, quarter = C / 4;
        std::vector<float> tx((size_t)w * half), ty((size_t)hh * half);
        auto fill = [&](std::vector<float>& tab, int n, double span) {
            // torch.linspace(-span*(n-1)/n, span*(n-1)/n, n) in float32
            const float lo = (float)(-span * (n - 1) / n), hi = (float)(span * (n - 1) / n);
            const float step = n > 1 ? (hi - lo) / (float)(n - 1) : 0.f;
            for (int i = 0; i < n; ++i) {
                const float pv = i < n / 2 ? lo + step * (float)i : hi - step * (float)(n - 1 - i);
                for (int j = 0; j < quarter; ++j) {
                    const double omega = 1.0 / pow(100.0, (double)j / (double)quarter);
                    const double a = (double)pv * omega;
                    tab[(size_t)i * half + j] = (float)sin(a) * 0.1f;
                    tab[(size_t)i * half + quarter + j] = (float)cos(a) * 0.1f;
                }
            }
        };
        fill(tx, w, sx);
        fill(ty, hh, sy);
        UvTab t{w, hh, C, nullptr, nullptr};
        int r2;
        if ((r2 = up(tx.data(), tx.size() * 4, (void**)&t.tx))) return r2;
        if ((r2 = up(ty.data(), ty.size() * 4, (void**)&t.ty))) return r2;
        t_->uv.push_back(t);
        return SKIMI_OK;
    };
    if (cfg.enable_depth || cfg.enable_point) {
        for (int i = 0; i < 4; ++i)
            if ((rc = add_uv(pw, ph, cfg.dpt_out_channels[i]))) return rc;
        if ((rc = add_uv(pw * p, ph * p, cfg.dpt_features / 2))) return rc;
    }
    *out = t_;
    entries.push_back(std::move(tabs));
    return SKIMI_OK;
}

static int forward_impl(skimi_vggt* h, Ctx& c, const float* images, const float* query, int B, int S, int H, int W, int nq,
                        const skimi_vggt_outputs* out) {
    const skimi_vggt_config& cfg = h->cfg;
    const int p = cfg.patch_size, C = cfg.embed_dim, ph = H / p, pw = W / p, np = ph * pw;
    const int nsp = 1 + cfg.num_register_tokens, P = nsp + np, F = B * S, M = F * P;
    const int prec = cfg.prec, adt = Ctx::act_dt(prec);
    const size_t es = Ctx::esz(adt);

    // split-K slab: large enough for the skinny camera-head / small-config GEMMs; the fp32-accurate contractions keep one
    // plane per K split (fixed summation order), so it holds several [M, N] planes of those
    c.slab_bytes = std::max<size_t>((size_t)F * 6 * C * 4 * 4 * 4, 4u << 20);
    c.slab = c.ar.alloc(c.slab_bytes);
    // zeroed once per forward; every split-K epilogue leaves the slab zero again
    c.zero(c.slab, c.slab_bytes);

    float* x = (float*)c.ar.alloc((size_t)M * C * 4);
    // kept intermediates
    std::vector<int> keep;
    auto want = [&](int l) { for (int k : keep) if (k == l) return; keep.push_back(l); };
    const bool run_depth = cfg.enable_depth && out && (out->depth || out->depth_conf);
    const bool run_point = cfg.enable_point && out && (out->world_points || out->world_points_conf);
    const bool run_cam = cfg.enable_camera && out && (out->pose_enc || out->pose_enc_list);
    const bool do_track = cfg.enable_track && out && out->track && query && nq > 0;
    if (run_depth || run_point || do_track) for (int i = 0; i < 4; ++i) want(cfg.dpt_layers[i]);
    if (run_cam || (out && out->tokens_last)) want(cfg.depth - 1);
    std::map<int, std::pair<float*, float*>> saved;
    for (int l : keep) {
        float* a = (float*)c.ar.alloc((size_t)M * C * 4);
        float* b = (float*)c.ar.alloc((size_t)M * C * 4);
        saved[l] = {a, b};
    }
    {
        const size_t mk = c.ar.mark();
        BlockBufs bb;
        bb.xn = c.ar.alloc((size_t)M * C * es + 256);     // + the zero page behind bf16x3 records (run_block)
        bb.qkv = c.ar.alloc((size_t)M * 3 * C * es);
        bb.ao = c.ar.alloc((size_t)M * C * es + 256);
        bb.hid = c.ar.alloc((size_t)M * 4 * C * es + 256);
        if (cfg.prec == SKIMI_PREC_FP8) {   // MXFP8 scratch of the widest quantised activation (the MLP hidden)
            const size_t kp = align_up((size_t)4 * C, 128);
            bb.q8 = c.ar.alloc((size_t)M * kp);
            bb.q8s = c.ar.alloc((size_t)M * (kp / 32));
        }
        // ---- patch embed (aggregator.py:195-208) ----
        void* pa = c.ar.alloc((size_t)F * np * h->patch_kp * es);
        c.run([&] { return patch_gather_launch(images, pa, adt, F, H, W, p, h->patch_kp, c.st); });
        {
            auto d = c.desc(h->patch_proj, pa, adt, h->patch_kp, F * np, x, SKIMI_F32, C);
            d.out_rows_per_batch = np; d.out_batch_stride = P; d.out_row_off = nsp;
            if (cfg.use_dino) {
                // + pos_embed[1 + p] (vision_transformer.py:221), broadcast over frames
                const bool native = H == W && H == cfg.dino_img_size;
                (void)native;
                d.resid = c.tabs ? c.tabs->dino_pos : h->dino_pos; d.ldr = C;   // dry run: any non-null pointer
                d.resid_rows_per_batch = np; d.resid_batch_stride = 0; d.resid_row_off = 1;
            }
            c.gemm(d);
        }
        if (cfg.use_dino) {
            c.run([&] { return special_tokens_launch(x, h->dino_special, F, S, P, nsp, C, c.st); });
            for (const BlockW& b : h->dino) run_block(c, b, x, F, P, C, cfg.dino_heads, 1e-6f, false, bb);
            // x_norm_patchtokens (vision_transformer.py:264-268): LayerNorm in place (row-local)
            c.ln(x, nullptr, C, M, C, h->dino_norm, 1e-6f, x, SKIMI_F32);
        }
        // camera / register tokens, frame 0 vs others (aggregator.py:210-217, 308-331)
        c.run([&] { return special_tokens_launch(x, h->agg_special, F, S, P, nsp, C, c.st); });
        // ---- alternating attention (aggregator.py:237-253) ----
        for (int i = 0; i < cfg.depth && !c.rc; ++i) {
            run_block(c, h->frame[i], x, F, P, C, cfg.num_heads, 1e-5f, true, bb);
            auto it = saved.find(i);
            if (it != saved.end()) c.copy(it->second.first, x, (size_t)M * C * 4);
            run_block(c, h->global[i], x, B, S * P, C, cfg.num_heads, 1e-5f, true, bb);
            if (it != saved.end()) c.copy(it->second.second, x, (size_t)M * C * 4);
        }
        c.ar.release(mk);
    }
    if (out && out->tokens_last)
        c.run([&] {
            // [B,S,P,2C] = cat(frame, global) of the last layer: two strided 2-D copies
            auto& sv = saved[cfg.depth - 1];
            if (hipMemcpy2DAsync(out->tokens_last, (size_t)2 * C * 4, sv.first, (size_t)C * 4, (size_t)C * 4, M,
                                 hipMemcpyDeviceToDevice, c.st) != hipSuccess ||
                hipMemcpy2DAsync(out->tokens_last + C, (size_t)2 * C * 4, sv.second, (size_t)C * 4, (size_t)C * 4, M,
                                 hipMemcpyDeviceToDevice, c.st) != hipSuccess) {
                set_error("hipMemcpy2DAsync failed");
                return (int)SKIMI_ERR_HIP;
            }
            return (int)SKIMI_OK;
        });
    if (run_cam) {
        auto& sv = saved[cfg.depth - 1];
        run_camera(c, h->cam, sv.first, sv.second, B, S, P, C, out->pose_enc_list, out->pose_enc);
    }
    float* sf[4];
    float* sg[4];
    if (run_depth || run_point || do_track)
        for (int i = 0; i < 4; ++i) {
            sf[i] = saved[cfg.dpt_layers[i]].first;
            sg[i] = saved[cfg.dpt_layers[i]].second;
        }
    if (run_depth) {
        float* pts = out->depth ? out->depth : (float*)c.ar.alloc((size_t)F * H * W * 4);
        float* cf = out->depth_conf ? out->depth_conf : (float*)c.ar.alloc((size_t)F * H * W * 4);
        run_dpt(c, h->depth, sf, sg, F, P, nsp, ph, pw, C, H, W, pts, cf, 0);
    }
    if (run_point) {
        float* pts = out->world_points ? out->world_points : (float*)c.ar.alloc((size_t)F * H * W * 3 * 4);
        float* cf = out->world_points_conf ? out->world_points_conf : (float*)c.ar.alloc((size_t)F * H * W * 4);
        run_dpt(c, h->point, sf, sg, F, P, nsp, ph, pw, C, H, W, pts, cf, 1);
    }
    if (do_track) run_track(c, sf, sg, B, S, P, nsp, ph, pw, C, H, W, query, nq, out->track, out->vis, out->conf);
    return c.rc;
}

// arena peaks of the calling thread's last skimi_vggt_forward: the sizing pass's and the real pass's (skimi_vggt_last_arena)
static thread_local size_t tl_arena_planned = 0, tl_arena_used = 0;

extern "C" {

skimi_vggt* skimi_vggt_create(const skimi_vggt_config* cfg) {
    if (!cfg) { set_error("skimi_vggt_create: null config"); return nullptr; }
    if (cfg->embed_dim <= 0 || cfg->num_heads <= 0 || cfg->embed_dim / cfg->num_heads != 64 ||
        cfg->embed_dim % cfg->num_heads != 0) {
        set_error("skimi_vggt_create: embed_dim / num_heads must be 64");
        return nullptr;
    }
    if (cfg->use_dino && cfg->embed_dim / cfg->dino_heads != 64) {
        set_error("skimi_vggt_create: DINOv2 head_dim must be 64");
        return nullptr;
    }
    if (cfg->patch_size <= 0 || cfg->depth <= 0 || cfg->num_register_tokens < 0) {
        set_error("skimi_vggt_create: bad sizes");
        return nullptr;
    }
    for (int i = 0; i < 4; ++i)
        if (cfg->dpt_layers[i] < 0 || cfg->dpt_layers[i] >= cfg->depth) {
            set_error("skimi_vggt_create: dpt_layers[%d] = %d outside [0, depth)", i, cfg->dpt_layers[i]);
            return nullptr;
        }
    if (cfg->prec < SKIMI_PREC_BF16 || cfg->prec > SKIMI_PREC_F16) {
        set_error("skimi_vggt_create: prec %d is not one of SKIMI_PREC_BF16 / BF16X3 / FP8 / F16", cfg->prec);
        return nullptr;
    }
    if (cfg->head_prec != SKIMI_PREC_BF16 && cfg->head_prec != SKIMI_PREC_BF16X3 && cfg->head_prec != SKIMI_PREC_F16) {
        set_error("skimi_vggt_create: head_prec %d: the depth / point heads run in SKIMI_PREC_BF16X3 (the reference's fp32) or, as a "
                  "faster, less accurate option, on SKIMI_PREC_F16 / SKIMI_PREC_BF16 operands", cfg->head_prec);
        return nullptr;
    }
    skimi_vggt* h = new skimi_vggt();
    h->cfg = *cfg;
    // SKIMI_DPT_FOLD=0: the heads' levels 0 / 1 as ConvTranspose GEMM + 3x3 conv (interleaved A/B timing, equivalence tests)
    h->dpt_fold = !(getenv("SKIMI_DPT_FOLD") && atoi(getenv("SKIMI_DPT_FOLD")) == 0);
    // SKIMI_DPT_OC1_COARSE=0: output_conv1 as the x2 upsample into records + the 3x3 conv on the fine map (same uses)
    h->dpt_oc1_coarse = !(getenv("SKIMI_DPT_OC1_COARSE") && atoi(getenv("SKIMI_DPT_OC1_COARSE")) == 0);
    return h;
}

void skimi_vggt_destroy(skimi_vggt* h) {
    if (!h) return;
    for (auto& kv : h->raw) (void)hipFree(kv.second.first);
    for (void* p : h->owned) (void)hipFree(p);
    h->tabs.clear();
    for (auto& kv : h->dino_pos_alt) (void)hipFree(kv.second);
    delete h;
}

int skimi_vggt_set_weight(skimi_vggt* h, const char* key, const float* data, int64_t n, int32_t on_device) {
    SKIMI_CHECK_ARG(h && key && data && n > 0, "skimi_vggt_set_weight: bad arguments");
    float* d = nullptr;
    SKIMI_HIP(hipMalloc((void**)&d, (size_t)n * 4));
    hipError_t e = hipMemcpy(d, data, (size_t)n * 4, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(d);
        set_error("skimi_vggt_set_weight: copy failed: %s", hipGetErrorString(e));
        return SKIMI_ERR_HIP;
    }
    auto it = h->raw.find(key);
    if (it != h->raw.end()) (void)hipFree(it->second.first);
    h->raw[key] = {d, n};
    h->finalized = false;
    return SKIMI_OK;
}

int skimi_vggt_set_pos_embed(skimi_vggt* h, int32_t H, int32_t W, const float* pos_embed, int32_t on_device) {
    SKIMI_CHECK_ARG(h && pos_embed && h->cfg.use_dino, "skimi_vggt_set_pos_embed: needs a DINOv2 model and a table");
    const int p = h->cfg.patch_size;
    SKIMI_CHECK_ARG(H > 0 && W > 0 && H % p == 0 && W % p == 0, "skimi_vggt_set_pos_embed: bad size %dx%d", H, W);
    const size_t n = ((size_t)(H / p) * (W / p) + 1) * h->cfg.embed_dim;
    float* d = nullptr;
    SKIMI_HIP(hipMalloc((void**)&d, n * 4));
    hipError_t e = hipMemcpy(d, pos_embed, n * 4, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(d);
        set_error("skimi_vggt_set_pos_embed: copy failed: %s", hipGetErrorString(e));
        return SKIMI_ERR_HIP;
    }
    // published under the handle's table lock; a table registered again for the same size replaces the
    // CONTENTS of the existing buffer (its address stays valid for forwards already enqueued)
    std::lock_guard<std::mutex> lk(h->prep_mu);
    auto it = h->dino_pos_alt.find({H, W});
    if (it != h->dino_pos_alt.end()) {
        e = hipMemcpy(it->second, d, n * 4, hipMemcpyDeviceToDevice);
        (void)hipFree(d);
        if (e != hipSuccess) {
            set_error("skimi_vggt_set_pos_embed: copy failed: %s", hipGetErrorString(e));
            return SKIMI_ERR_HIP;
        }
        return SKIMI_OK;
    }
    h->dino_pos_alt[{H, W}] = d;
    return SKIMI_OK;
}

int skimi_vggt_finalize(skimi_vggt* h) {
    SKIMI_CHECK_ARG(h, "skimi_vggt_finalize: null handle");
    for (void* p : h->owned) (void)hipFree(p);
    h->owned.clear();
    int rc;
    if ((rc = pack_model(h))) return rc;
    // release the staged fp32 copies
    for (auto it = h->raw.begin(); it != h->raw.end();) {
        (void)hipFree(it->second.first);
        it = h->raw.erase(it);
    }
    h->finalized = true;
    return SKIMI_OK;
}

static int check_shape(const skimi_vggt* h, int B, int S, int H, int W) {
    SKIMI_CHECK_ARG(B > 0 && S > 0, "skimi_vggt: B and S must be positive");
    const int p = h->cfg.patch_size;
    // patch_embed.py:69-70
    SKIMI_CHECK_ARG(H > 0 && H % p == 0, "Input image height %d is not a multiple of patch height %d", H, p);
    SKIMI_CHECK_ARG(W > 0 && W % p == 0, "Input image width %d is not a multiple of patch width: %d", W, p);
    if (h->cfg.use_dino && !(H == W && H == h->cfg.dino_img_size)) {
        std::lock_guard<std::mutex> lk(const_cast<skimi_vggt*>(h)->prep_mu);
        SKIMI_CHECK_ARG(h->dino_pos_alt.count({H, W}) != 0,
                        "DINOv2 pos_embed for %dx%d (model built for %d) has not been registered: call "
                        "skimi_vggt_set_pos_embed with the bicubic-antialias resized table first", H, W,
                        h->cfg.dino_img_size);
    }
    return SKIMI_OK;
}

size_t skimi_vggt_workspace_bytes(skimi_vggt* h, int32_t B, int32_t S, int32_t H, int32_t W, int32_t n_query) {
    if (!h || check_shape(h, B, S, H, W)) return 0;
    Ctx c{h, nullptr};
    c.ar.dry = true;
    skimi_vggt_outputs all;
    memset(&all, 0, sizeof all);
    // assume every enabled head runs and writes straight to caller buffers
    float* one = (float*)(uintptr_t)16;
    all.pose_enc = all.pose_enc_list = all.depth = all.depth_conf = all.world_points = all.world_points_conf = one;
    all.tokens_last = one;
    if (n_query > 0) all.track = all.vis = all.conf = one;
    forward_impl(h, c, nullptr, n_query > 0 ? one : nullptr, B, S, H, W, n_query, &all);
    return align_up(c.ar.peak, 256) + 256;
}

int skimi_vggt_rope_positions(skimi_vggt* h, int32_t frames, int32_t H, int32_t W, int32_t* positions) {
    SKIMI_CHECK_ARG(h && positions && frames > 0, "skimi_vggt_rope_positions: bad arguments");
    int rc;
    if ((rc = check_shape(h, 1, frames, H, W))) return rc;
    const ShapeTabs* tabs = nullptr;
    {
        std::lock_guard<std::mutex> lk(h->prep_mu);
        if ((rc = prepare(h, frames, frames, H, W, &tabs))) return rc;
    }
    const int p = h->cfg.patch_size;
    const size_t P = 1 + h->cfg.num_register_tokens + (size_t)(H / p) * (W / p);
    SKIMI_HIP(hipMemcpy(positions, tabs->pos, (size_t)frames * P * 2 * sizeof(int32_t), hipMemcpyDeviceToDevice));
    return SKIMI_OK;
}

int skimi_vggt_forward(skimi_vggt* h, const float* images, const float* query_points, int32_t B, int32_t S, int32_t H,
                       int32_t W, int32_t n_query, const skimi_vggt_outputs* out, void* workspace,
                       size_t workspace_bytes, void* stream) {
    SKIMI_CHECK_ARG(h && images && out && workspace, "skimi_vggt_forward: null argument");
    if (!h->finalized) {
        set_error("skimi_vggt_forward: weights not finalized");
        return SKIMI_ERR_STATE;
    }
    int rc;
    if ((rc = check_shape(h, B, S, H, W))) return rc;
    // Calls of any shapes may run at the same time from several host threads (own workspace and stream
    // each): the per-shape tables are a keyed cache of immutable entries that live as long as the handle.
    const ShapeTabs* tabs = nullptr;
    {
        std::lock_guard<std::mutex> lk(h->prep_mu);
        if ((rc = prepare(h, B * S, S, H, W, &tabs))) return rc;
    }
    Ctx c{h, (hipStream_t)stream};
    c.tabs = tabs;
    c.ar.base = (char*)workspace;
    c.ar.cap = workspace_bytes;
    // refuse before launching anything if the arena cannot hold the plan
    {
        Ctx dry{h, nullptr};
        dry.ar.dry = true;
        forward_impl(h, dry, images, query_points, B, S, H, W, n_query, out);
        if (dry.ar.peak > workspace_bytes) {
            set_error("skimi_vggt_forward: workspace %zu < %zu", workspace_bytes, dry.ar.peak);
            return SKIMI_ERR_WORKSPACE;
        }
        tl_arena_planned = dry.ar.peak;
    }
    rc = forward_impl(h, c, images, query_points, B, S, H, W, n_query, out);
    tl_arena_used = c.ar.peak;
    return rc;
}

int skimi_vggt_last_arena(uint64_t* planned, uint64_t* used) {
    SKIMI_CHECK_ARG(planned && used, "skimi_vggt_last_arena: null argument");
    *planned = tl_arena_planned;
    *used = tl_arena_used;
    return SKIMI_OK;
}

int32_t skimi_vggt_oc1_coarse_count(void) { return dpt_oc1_coarse_count(); }

}  // extern "C"
