// Camera head of the VGGT forward (vggt/vggt/heads/camera_head.py:73-141): iterative pose refinement on the camera
// token of the last [frame | global] intermediate.
#include "vggt_kernels.h"
#include "vggt_model.h"

namespace skimi {
namespace vggt {

// camera head (vggt/vggt/heads/camera_head.py:73-141), fp32 activations
void run_camera(Ctx& c, const CamW& w, const float* sf, const float* sg, int B, int S, int P, int C, float* out_list,
                float* out_last) {
    const skimi_vggt_config& cfg = c.h->cfg;
    const int R = B * S, D = 2 * C;
    const size_t mk = c.ar.mark();
    float* pose_tokens = (float*)c.ar.alloc((size_t)R * D * 4);
    float* xn = (float*)c.ar.alloc((size_t)R * D * 4);
    float* xc = (float*)c.ar.alloc((size_t)R * D * 4);
    float* e = (float*)c.ar.alloc((size_t)R * D * 4);
    float* mod = (float*)c.ar.alloc((size_t)R * 3 * D * 4);
    float* pred16 = (float*)c.ar.alloc((size_t)R * 16 * 4);
    float* t2 = (float*)c.ar.alloc((size_t)R * (D / 2) * 4);
    float* delta = (float*)c.ar.alloc((size_t)R * 9 * 4);
    BlockBufs bb;
    bb.xn = c.ar.alloc((size_t)R * D * 4 + 256);     // + the zero page behind bf16x3 records (run_block)
    bb.qkv = c.ar.alloc((size_t)R * 3 * D * 4);
    bb.ao = c.ar.alloc((size_t)R * D * 4 + 256);
    bb.hid = c.ar.alloc((size_t)R * 4 * D * 4 + 256);
    // camera token = token 0 of every frame of the last [frame | global] intermediate
    c.ln(sf, sg, (long)P * C, R, D, w.token_norm, 1e-5f, pose_tokens, SKIMI_F32);
    LNw none;
    for (int it = 0; it < cfg.cam_iters; ++it) {
        if (it == 0) c.run([&] { return tile_vec_launch(w.empty16, pred16, 16, R, c.st); });
        {
            auto d = c.desc(w.embed_pose, pred16, SKIMI_F32, 16, R, e, SKIMI_F32, D);
            d.act = SKIMI_ACT_SILU;   // poseLN_modulation = Sequential(SiLU, Linear)
            c.gemm(d);
        }
        {
            auto d = c.desc(w.poseLN, e, SKIMI_F32, D, R, mod, SKIMI_F32, 3 * D);
            c.gemm(d);
        }
        c.ln(pose_tokens, nullptr, D, R, D, none, 1e-6f, xn, SKIMI_F32);
        c.run([&] { return adaln_launch(xn, pose_tokens, mod, xc, R, D, c.st); });
        for (const BlockW& b : w.trunk) run_block(c, b, xc, B, S, D, cfg.cam_heads, 1e-5f, false, bb);
        c.ln(xc, nullptr, D, R, D, w.trunk_norm, 1e-5f, xn, SKIMI_F32);
        {
            auto d = c.desc(w.fc1, xn, SKIMI_F32, D, R, t2, SKIMI_F32, D / 2);
            d.act = SKIMI_ACT_GELU;
            c.gemm(d);
        }
        {
            auto d = c.desc(w.fc2, t2, SKIMI_F32, D / 2, R, delta, SKIMI_F32, 9);
            c.gemm(d);
        }
        float* dst = out_list ? out_list + (size_t)it * R * 9 : (it == cfg.cam_iters - 1 ? out_last : xn /*scratch*/);
        c.run([&] { return pose_update_launch(delta, pred16, dst, R, it == 0, c.st); });
        if (it == cfg.cam_iters - 1 && out_list && out_last) c.copy(out_last, dst, (size_t)R * 9 * 4);
    }
    c.ar.release(mk);
}

}  // namespace vggt
}  // namespace skimi
