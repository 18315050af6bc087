// VGGT weights, packed once: what skimi_vggt_finalize makes of the staged fp32 state_dict (conv taps ->
// [Cout, ky, kx, Cin], ConvTranspose -> pixel-shuffle GEMM, bf16 / fp16 / MXFP8 copies, bf16x3 records, K padded to 8).
// Modules as built by vggt/vggt/models/vggt.py:22-27, models/aggregator.py:52-182, heads/dpt_head.py:43-113
// (fusion blocks :347-430) and heads/camera_head.py:26-71; the track head's are packed in vggt_track.hip.
#include <stdlib.h>

#include "env.h"
#include "gemm_epilogue.h"
#include "kernels.h"
#include "vggt_kernels.h"
#include "vggt_model.h"

namespace skimi {
namespace vggt {

float* Packer::raw(const std::string& key, int64_t n) {
    if (rc) return nullptr;
    auto it = h->raw.find(key);
    if (it == h->raw.end()) {
        set_error("skimi_vggt_finalize: missing weight '%s'", key.c_str());
        rc = SKIMI_ERR_STATE;
        return nullptr;
    }
    if (it->second.second != n) {
        set_error("skimi_vggt_finalize: weight '%s' has %ld elements, expected %ld", key.c_str(),
                  (long)it->second.second, (long)n);
        rc = SKIMI_ERR_STATE;
        return nullptr;
    }
    return it->second.first;
}
void* Packer::dmalloc(size_t bytes) {
    if (rc) return nullptr;
    void* p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess) {
        set_error("skimi_vggt_finalize: hipMalloc(%zu) failed", bytes);
        rc = SKIMI_ERR_HIP;
        return nullptr;
    }
    h->owned.push_back(p);
    return p;
}
// a plain fp32 parameter used as is (LN affine, bias, LayerScale, tokens): private copy
float* Packer::keep(const std::string& key, int64_t n) {
    float* src = raw(key, n);
    if (!src) return nullptr;
    float* dst = (float*)dmalloc(n * 4);
    if (dst && hipMemcpyAsync(dst, src, n * 4, hipMemcpyDeviceToDevice, st) != hipSuccess) rc = SKIMI_ERR_HIP;
    return dst;
}

// matrix [N, K] fp32 on device (owned by caller) -> Lin in the requested precision, K padded to 8
Lin Packer::pack_matrix(float* src, int N, int K, int prec) {
    Lin L;
    L.N = N;
    L.K = (int)align_up((size_t)K, 8);
    L.prec = prec;
    if (rc) return L;
    float* m = src;
    if (L.K != K) {
        m = (float*)dmalloc((size_t)N * L.K * 4);
        if (m && (rc = pad_cols_launch(src, m, N, K, L.K, st))) return L;
    }
    if (prec == SKIMI_PREC_BF16 || prec == SKIMI_PREC_F16) {
        void* b = dmalloc((size_t)N * L.K * 2);
        if (b) rc = prec == SKIMI_PREC_F16 ? f32_to_f16_launch(m, b, (long)N * L.K, st) : f32_to_bf16_launch(m, b, (long)N * L.K, st);
        L.w = b;
        L.wdt = prec == SKIMI_PREC_F16 ? SKIMI_F16 : SKIMI_BF16;
    } else {
        if (m == src) {   // private copy: the staged buffer is released after finalize
            m = (float*)dmalloc((size_t)N * L.K * 4);
            if (m && hipMemcpyAsync(m, src, (size_t)N * L.K * 4, hipMemcpyDeviceToDevice, st) != hipSuccess)
                rc = SKIMI_ERR_HIP;
        }
        L.w = m;
        L.wdt = SKIMI_F32;
    }
    return L;
}
Lin Packer::linear(const std::string& p, int N, int K, int prec, bool bias) {
    Lin L = pack_matrix(raw(p + ".weight", (int64_t)N * K), N, K, prec);
    if (bias) L.b = keep(p + ".bias", N);
    return L;
}
// nn.MultiheadAttention style names
Lin Packer::linear_named(const std::string& wkey, const std::string& bkey, int N, int K, int prec) {
    Lin L = pack_matrix(raw(wkey, (int64_t)N * K), N, K, prec);
    L.b = keep(bkey, N);
    return L;
}
// bf16 [hi 32 | lo 32] records of a packed fp32 matrix, for the LDS-DMA bf16x3 kernel (which
// gemm_x3dma_eligible then picks for launches that fill the chip with 256-row tiles)
void Packer::add_records(Lin& L) {
    const size_t n = (size_t)L.N * ((L.K + 31) / 32 * 32);
    L.w_split = dmalloc(n * 4);
    if (L.w_split) rc = split_records_launch((const float*)L.w, L.K, L.N, L.K, L.w_split, st);
}
ConvW Packer::conv(const std::string& p, int Co, int Ci, int k, int stride, int pad, int prec, bool bias) {
    ConvW c;
    c.k = k; c.stride = stride; c.pad = pad; c.cin = Ci;
    float* src = raw(p + ".weight", (int64_t)Co * Ci * k * k);
    if (rc) return c;
    float* perm = src;
    float* tmp = nullptr;
    if (k > 1) {
        // fp32-accurate convs run on K-tiles of 32: order K slice-major there (see permute_conv_kernel)
        const int force_tap_major = (int)env_once("SKIMI_CONV_TAP_MAJOR", 0);   // A/B timing
        c.kmode = (prec == SKIMI_PREC_BF16X3 && Ci % 32 == 0 && !force_tap_major) ? 2 : 1;
        if (hipMalloc((void**)&tmp, (size_t)Co * Ci * k * k * 4) != hipSuccess) { rc = SKIMI_ERR_HIP; return c; }
        if ((rc = permute_conv_launch(src, tmp, Co, Ci, k, k, st, c.kmode == 2))) return c;
        perm = tmp;
    }
    c.lin = pack_matrix(perm, Co, Ci * k * k, prec);
    // fp32-accurate 3x3 convs, wide 1x1 projections and the ConvTranspose matrices also get bf16
    // hi|lo records: the LDS-DMA bf16x3 kernel (gemm_x3dma.hip) beats the generic one wherever
    // 256-row tiles fill the chip
    if (!rc && prec == SKIMI_PREC_BF16X3 && Ci % 32 == 0 && ((k == 3 && Co >= 96) || (k == 1 && Co >= 512)))
        add_records(c.lin);
    if (tmp) { (void)hipStreamSynchronize(st); (void)hipFree(tmp); }
    if (bias) c.lin.b = keep(p + ".bias", Co);
    return c;
}
// ConvTranspose2d(C, C, k = s, stride = s): [(a,b,co), Ci] weight, bias tiled s*s times
Lin Packer::convT(const std::string& p, int C, int s, int prec) {
    Lin L;
    float* src = raw(p + ".weight", (int64_t)C * C * s * s);
    float* bsrc = raw(p + ".bias", C);
    if (rc) return L;
    float* tmp = nullptr;
    if (hipMalloc((void**)&tmp, (size_t)C * C * s * s * 4) != hipSuccess) { rc = SKIMI_ERR_HIP; return L; }
    if ((rc = permute_convT_launch(src, tmp, C, C, s, st))) return L;
    L = pack_matrix(tmp, s * s * C, C, prec);
    if (!rc && prec == SKIMI_PREC_BF16X3 && C % 32 == 0) add_records(L);
    (void)hipStreamSynchronize(st);
    (void)hipFree(tmp);
    L.b = (float*)dmalloc((size_t)s * s * C * 4);
    if (L.b) rc = rc ? rc : tile_vec_launch(bsrc, L.b, C, s * s, st);
    return L;
}
// a 3x3 conv's taps as nine stacked 1x1 matrices [9 * Co][Ci] (row t * Co + k = W[k, :, ty, tx], t = 3 ty + tx), with
// bf16x3 records and no bias: the form the DPT heads contract on the coarse map in front of a bilinear upsample
Lin Packer::conv_taps(const std::string& p, int Co, int Ci) {
    Lin L;
    float* src = raw(p + ".weight", (int64_t)Co * Ci * 9);
    if (rc) return L;
    float* tmp = nullptr;
    if (hipMalloc((void**)&tmp, (size_t)9 * Co * Ci * 4) != hipSuccess) { rc = SKIMI_ERR_HIP; return L; }
    if (!(rc = permute_conv_taps_launch(src, tmp, Co, Ci, 3, 3, st))) {
        L = pack_matrix(tmp, 9 * Co, Ci, SKIMI_PREC_BF16X3);
        if (!rc) add_records(L);
    }
    (void)hipStreamSynchronize(st);
    (void)hipFree(tmp);
    return L;
}
// resize_layers[i] (ConvTranspose2d(C, C, k = s, stride = s)) folded into layer{i+1}_rn (3x3, C -> Co, no bias): the
// per-phase matrices as weight records + the 9 border classes of the folded bias, from the staged fp32 weights
// (float64 sums, one rounding).  K = 4 C is the longest phase; the kernel derives each phase's own from its taps.
Lin Packer::conv_fold(const std::string& pT, const std::string& pRn, int C, int Co, int s) {
    Lin L;
    L.N = Co; L.K = 4 * C; L.prec = SKIMI_PREC_BF16X3; L.wdt = SKIMI_F32;
    float* wT = raw(pT + ".weight", (int64_t)C * C * s * s);
    float* bT = raw(pT + ".bias", C);
    float* wrn = raw(pRn + ".weight", (int64_t)Co * C * 9);
    if (rc) return L;
    const size_t n = (size_t)(s + 2) * (s + 2) * Co * C;
    float* tmp = nullptr;
    if (hipMalloc((void**)&tmp, n * 4) != hipSuccess) { rc = SKIMI_ERR_HIP; return L; }
    L.w_split = dmalloc(n * 4);
    L.b = (float*)dmalloc((size_t)9 * Co * 4);
    L.w = L.w_split;   // the descriptor's W: this form has no plain fp32 matrix
    if (!rc) rc = dpt_fold_pack_launch(wT, bT, wrn, C, C, Co, s, tmp, L.w_split, L.b, st);
    (void)hipStreamSynchronize(st);
    (void)hipFree(tmp);
    return L;
}
// MXFP8 copy of a packed Linear (from the staged fp32 weights: one rounding)
void Packer::add_fp8(Lin& L, const std::string& p, int N, int K) {
    if (rc) return;
    const size_t Kp = align_up((size_t)K, 128);
    L.wq = dmalloc((size_t)N * Kp);
    L.wq_scales = dmalloc((size_t)N * (Kp / 32));
    if (L.wq && L.wq_scales) rc = quant_mx_launch(raw(p + ".weight", (int64_t)N * K), SKIMI_F32, K, N, K, L.wq, L.wq_scales, st);
}
BlockW Packer::block(const std::string& p, int C, int hidden, bool qk_norm, int hd, int prec_in) {
    BlockW b;
    const bool fp8 = prec_in == SKIMI_PREC_FP8 && C % 32 == 0 && hidden % 32 == 0;
    const int prec = prec_in == SKIMI_PREC_FP8 ? SKIMI_PREC_BF16 : prec_in;
    b.n1 = ln(p + ".norm1", C);
    b.n2 = ln(p + ".norm2", C);
    b.qkv = linear(p + ".attn.qkv", 3 * C, C, prec);
    b.proj = linear(p + ".attn.proj", C, C, prec);
    b.fc1 = linear(p + ".mlp.fc1", hidden, C, prec);
    b.fc2 = linear(p + ".mlp.fc2", C, hidden, prec);
    // fp32-accurate mode: the four Linears also as bf16x3 records, so that launches that fill the chip with 256-row
    // tiles (from one 8-view time step on) run on the LDS-DMA bf16x3 kernel (gemm_x3dma.hip) instead of the generic one
    if (!rc && prec == SKIMI_PREC_BF16X3 && C % 32 == 0 && hidden % 32 == 0) {
        add_records(b.qkv);
        add_records(b.proj);
        add_records(b.fc1);
        add_records(b.fc2);
    }
    if (fp8) {
        add_fp8(b.qkv, p + ".attn.qkv", 3 * C, C);
        // SKIMI_FP8_PROJ=0 (read when the weights are packed): proj stays on the bf16 kernel, as in round 2 (A/B timing)
        if (!(getenv("SKIMI_FP8_PROJ") && atoi(getenv("SKIMI_FP8_PROJ")) == 0)) add_fp8(b.proj, p + ".attn.proj", C, C);
        add_fp8(b.fc1, p + ".mlp.fc1", hidden, C);
        add_fp8(b.fc2, p + ".mlp.fc2", C, hidden);
    }
    b.ls1 = keep(p + ".ls1.gamma", C);
    b.ls2 = keep(p + ".ls2.gamma", C);
    if (qk_norm) {
        b.qn_w = keep(p + ".attn.q_norm.weight", hd);
        b.qn_b = keep(p + ".attn.q_norm.bias", hd);
        b.kn_w = keep(p + ".attn.k_norm.weight", hd);
        b.kn_b = keep(p + ".attn.k_norm.bias", hd);
    }
    return b;
}
DptW Packer::dpt(const std::string& p, int D, int features, const int* oc, int n_out, bool feature_only, int prec) {
    DptW d;
    d.features = features;
    d.n_out = n_out;
    d.feature_only = feature_only;
    for (int i = 0; i < 4; ++i) d.oc[i] = oc[i];
    d.norm = ln(p + ".norm", D);
    for (int i = 0; i < 4; ++i) {
        d.proj[i] = linear(p + ".projects." + std::to_string(i), oc[i], D, prec);
        if (!rc && prec == SKIMI_PREC_BF16X3 && oc[i] >= 512 && D % 32 == 0) add_records(d.proj[i]);
    }
    d.rs0 = convT(p + ".resize_layers.0", oc[0], 4, prec);
    d.rs1 = convT(p + ".resize_layers.1", oc[1], 2, prec);
    d.rs3 = conv(p + ".resize_layers.3", oc[3], oc[3], 3, 2, 1, prec, true);
    for (int i = 0; i < 4; ++i)
        d.rn[i] = conv(p + ".scratch.layer" + std::to_string(i + 1) + "_rn", features, oc[i], 3, 1, 1, prec, false);
    // the unfolded rs0 / rs1 / rn[0..1] stay packed: launches too small for the 256-row kernel take them
    if (h->dpt_fold && prec == SKIMI_PREC_BF16X3 && features % 32 == 0 && features > 128)
        for (int i = 0; i < 2; ++i)
            if (oc[i] % 32 == 0)
                d.fold[i] = conv_fold(p + ".resize_layers." + std::to_string(i), p + ".scratch.layer" + std::to_string(i + 1) + "_rn",
                                      oc[i], features, i == 0 ? 4 : 2);
    for (int r = 0; r < 4; ++r) {
        const std::string rp = p + ".scratch.refinenet" + std::to_string(r + 1);
        FusionW& f = d.ref[r];
        f.out_conv = linear(rp + ".out_conv", features, features, prec);
        if (!rc && prec == SKIMI_PREC_BF16X3 && features % 32 == 0) add_records(f.out_conv);
        f.has_r1 = r != 3;
        if (f.has_r1) {
            f.r1c1 = conv(rp + ".resConfUnit1.conv1", features, features, 3, 1, 1, prec, true);
            f.r1c2 = conv(rp + ".resConfUnit1.conv2", features, features, 3, 1, 1, prec, true);
        }
        f.r2c1 = conv(rp + ".resConfUnit2.conv1", features, features, 3, 1, 1, prec, true);
        f.r2c2 = conv(rp + ".resConfUnit2.conv2", features, features, 3, 1, 1, prec, true);
    }
    if (feature_only) {
        d.oc1 = conv(p + ".scratch.output_conv1", features, features, 3, 1, 1, prec, true);
    } else {
        d.oc1 = conv(p + ".scratch.output_conv1", features / 2, features, 3, 1, 1, prec, true);
        // the 3x3 form stays packed: launches too small for the 256-row kernel take it
        if (h->dpt_oc1_coarse && prec == SKIMI_PREC_BF16X3 && features % 32 == 0)
            d.oc1t = conv_taps(p + ".scratch.output_conv1", features / 2, features);
        d.oc2a = conv(p + ".scratch.output_conv2.0", 32, features / 2, 3, 1, 1, prec, true);
        if (!rc && prec == SKIMI_PREC_BF16X3 && (features / 2) % 32 == 0) {
            // the full-resolution 3x3 -> 32 conv runs as a direct convolution (conv_direct.hip)
            const int Ci = features / 2;
            float* src = raw(p + ".scratch.output_conv2.0.weight", (int64_t)32 * Ci * 9);
            d.oc2a_direct = (unsigned short*)dmalloc((size_t)32 * Ci * 9 * 2 * 2);
            if (!rc && d.oc2a_direct) rc = conv_direct_pack_launch(src, d.oc2a_direct, Ci, st);
            if (!rc && hipStreamSynchronize(st) != hipSuccess) rc = SKIMI_ERR_HIP;
        }
        d.oc2b_w = keep(p + ".scratch.output_conv2.2.weight", (int64_t)n_out * 32);
        d.oc2b_b = keep(p + ".scratch.output_conv2.2.bias", n_out);
    }
    return d;
}

// the whole model from the handle's staged weights; returns once the packing kernels have finished
int pack_model(skimi_vggt* h) {
    const skimi_vggt_config& cfg = h->cfg;
    Packer pk{h};
    const int C = cfg.embed_dim, p = cfg.patch_size, R = cfg.num_register_tokens, nsp = 1 + R;
    const int hidden = 4 * C, D = 2 * C;
    const std::string A = "aggregator";
    const int kraw = 3 * p * p;
    // ---- patch embed ----
    const std::string pe = cfg.use_dino ? A + ".patch_embed.patch_embed.proj" : A + ".patch_embed.proj";
    h->patch_proj = pk.linear(pe, C, kraw, cfg.prec == SKIMI_PREC_FP8 ? SKIMI_PREC_BF16 : cfg.prec);   // FP8 mode: only the block Linears are MXFP8
    h->patch_kp = h->patch_proj.K;
    if (cfg.use_dino) {
        const std::string d = A + ".patch_embed";
        const int g = cfg.dino_img_size / p, np0 = g * g;
        h->dino_pos = pk.keep(d + ".pos_embed", (int64_t)(np0 + 1) * C);
        float* cls = pk.raw(d + ".cls_token", C);
        float* reg = R ? pk.raw(d + ".register_tokens", (int64_t)R * C) : nullptr;
        (void)pk.raw(d + ".mask_token", C);   // present in the state_dict, unused in inference
        h->dino_special = (float*)pk.dmalloc((size_t)2 * nsp * C * 4);
        if (!pk.rc) {
            // row 0 = cls + pos_embed[0] (vision_transformer.py:220-221), rows 1..R = registers
            std::vector<float> hc(C), hp(C), hr((size_t)R * C), tab((size_t)2 * nsp * C);
            SKIMI_HIP(hipMemcpy(hc.data(), cls, C * 4, hipMemcpyDeviceToHost));
            SKIMI_HIP(hipMemcpy(hp.data(), h->dino_pos, C * 4, hipMemcpyDeviceToHost));
            if (R) SKIMI_HIP(hipMemcpy(hr.data(), reg, (size_t)R * C * 4, hipMemcpyDeviceToHost));
            for (int s = 0; s < 2; ++s) {
                for (int c = 0; c < C; ++c) tab[((size_t)s * nsp) * C + c] = hc[c] + hp[c];
                for (int r = 0; r < R; ++r)
                    for (int c = 0; c < C; ++c) tab[((size_t)s * nsp + 1 + r) * C + c] = hr[(size_t)r * C + c];
            }
            SKIMI_HIP(hipMemcpy(h->dino_special, tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
        }
        h->dino.clear();
        for (int i = 0; i < cfg.dino_depth; ++i)
            h->dino.push_back(pk.block(d + ".blocks." + std::to_string(i), C, hidden, false, 64, cfg.prec));
        h->dino_norm = pk.ln(d + ".norm", C);
    }
    // camera_token [1,2,1,C], register_token [1,2,R,C] -> table [2][1+R][C]
    {
        float* cam = pk.raw(A + ".camera_token", (int64_t)2 * C);
        float* reg = R ? pk.raw(A + ".register_token", (int64_t)2 * R * C) : nullptr;
        h->agg_special = (float*)pk.dmalloc((size_t)2 * nsp * C * 4);
        if (!pk.rc) {
            for (int s = 0; s < 2; ++s) {
                SKIMI_HIP(hipMemcpy(h->agg_special + (size_t)s * nsp * C, cam + (size_t)s * C, C * 4, hipMemcpyDeviceToDevice));
                if (R) SKIMI_HIP(hipMemcpy(h->agg_special + ((size_t)s * nsp + 1) * C, reg + (size_t)s * R * C,
                                           (size_t)R * C * 4, hipMemcpyDeviceToDevice));
            }
        }
    }
    h->frame.clear();
    h->global.clear();
    for (int i = 0; i < cfg.depth; ++i) h->frame.push_back(pk.block(A + ".frame_blocks." + std::to_string(i), C, hidden, true, 64, cfg.prec));
    for (int i = 0; i < cfg.depth; ++i) h->global.push_back(pk.block(A + ".global_blocks." + std::to_string(i), C, hidden, true, 64, cfg.prec));
    // ---- camera head: fp32 (BF16X3) always ----
    if (cfg.enable_camera) {
        const std::string Hc = "camera_head";
        const int X3 = SKIMI_PREC_BF16X3;
        h->cam.trunk.clear();
        for (int i = 0; i < cfg.cam_trunk_depth; ++i)
            h->cam.trunk.push_back(pk.block(Hc + ".trunk." + std::to_string(i), D, 4 * D, false, 0, X3));
        h->cam.token_norm = pk.ln(Hc + ".token_norm", D);
        h->cam.trunk_norm = pk.ln(Hc + ".trunk_norm", D);
        float* ept = pk.raw(Hc + ".empty_pose_tokens", 9);
        h->cam.empty16 = (float*)pk.dmalloc(16 * 4);
        if (!pk.rc) pk.rc = pad_cols_launch(ept, h->cam.empty16, 1, 9, 16, pk.st);
        h->cam.embed_pose = pk.linear(Hc + ".embed_pose", D, 9, X3);   // K padded to 16
        h->cam.poseLN = pk.linear(Hc + ".poseLN_modulation.1", 3 * D, D, X3);
        h->cam.fc1 = pk.linear(Hc + ".pose_branch.fc1", D / 2, D, X3);
        h->cam.fc2 = pk.linear(Hc + ".pose_branch.fc2", 9, D / 2, X3);
    }
    if (cfg.enable_point) h->point = pk.dpt("point_head", D, cfg.dpt_features, cfg.dpt_out_channels, 4, false, cfg.head_prec);
    if (cfg.enable_depth) h->depth = pk.dpt("depth_head", D, cfg.dpt_features, cfg.dpt_out_channels, 2, false, cfg.head_prec);
    if (cfg.enable_track) pack_track(pk, h);
    if (pk.rc) return pk.rc;
    SKIMI_HIP(hipStreamSynchronize(pk.st));
    return SKIMI_OK;
}

}  // namespace vggt
}  // namespace skimi
