// What the parts of the VGGT forward share (vggt.hip and vggt_*.hip): the packed weights, the handle, the weight
// packer, the forward context with its bump arena, and the parts' entry points.  Host code only; nothing in here is
// part of the C API (include/skimi.h sees `struct skimi_vggt` as an opaque type).
#pragma once
#include <string.h>

#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "common.h"

namespace skimi {
namespace vggt {

struct Lin {              // out = A . W^T (+ b)
    void* w = nullptr;    // [N, ldw] bf16 or f32
    int wdt = SKIMI_F32;
    float* b = nullptr;
    int N = 0, K = 0;     // K as seen by the GEMM (padded)
    int prec = SKIMI_PREC_BF16X3;
    void* w_split = nullptr;   // BF16X3 only: bf16 [hi 32 | lo 32] records for the LDS-DMA kernel (wide 3x3 convs)
    void* wq = nullptr;        // SKIMI_PREC_FP8 blocks: the same matrix as MXFP8 payload [N][Kp] + scales [N][Kp / 32]
    void* wq_scales = nullptr;
};
struct LNw { float* g = nullptr; float* b = nullptr; };
struct BlockW {
    LNw n1, n2;
    Lin qkv, proj, fc1, fc2;
    float *ls1 = nullptr, *ls2 = nullptr;
    float *qn_w = nullptr, *qn_b = nullptr, *kn_w = nullptr, *kn_b = nullptr;
};
struct ConvW { Lin lin; int k = 1, stride = 1, pad = 0, cin = 0; int kmode = 1; };   // kmode: a_mode of the gather (1 tap-major, 2 slice-major K)
struct FusionW { Lin out_conv; ConvW r1c1, r1c2, r2c1, r2c2; bool has_r1 = false; };
struct DptW {
    LNw norm;
    Lin proj[4];
    Lin rs0, rs1;       // ConvTranspose k=s=4 / 2 as pixel-shuffle GEMMs (bias tiled s*s times)
    Lin fold[2];        // rs0 . rn[0] and rs1 . rn[1] folded per output phase (dpt_fold_pack_launch): w_split = the phase
                        // matrices' records, b = beta [9][features]; w_split NULL = not folded (SKIMI_DPT_FOLD=0, 16-bit heads)
    ConvW rs3;
    ConvW rn[4];
    FusionW ref[4];     // ref[0] = refinenet1 ... ref[3] = refinenet4
    ConvW oc1, oc2a;
    Lin oc1t;           // output_conv1's nine taps as 1x1 matrices, [9 * features / 2][features] (row t * features / 2 + k =
                        // W[k, :, ty, tx]), no bias: contracted on refinenet1's coarse map, the x2 upsample then sums the taps
                        // (dpt_tap_sum_launch); w_split NULL = not packed (SKIMI_DPT_OC1_COARSE=0, feature_only, 16-bit heads)
    float *oc2b_w = nullptr, *oc2b_b = nullptr;
    unsigned short* oc2a_direct = nullptr;   // conv_direct.hip weight layout of oc2a (fp32-accurate heads)
    int n_out = 0, features = 0, oc[4] = {0, 0, 0, 0};
    bool feature_only = false, pos_embed = true;
    bool out_f32 = false;   // feature_only heads: the returned feature map is fp32 whatever the activation format (the tracker reads fp32)
    const LNw* out_ln = nullptr;   // feature_only heads with 128 features: LayerNorm applied by the last upsample (the tracker's fmap_norm)
    int down_ratio = 1;
};
struct CamW {
    std::vector<BlockW> trunk;
    LNw token_norm, trunk_norm;
    float* empty16 = nullptr;   // empty_pose_tokens padded to 16
    Lin embed_pose, poseLN, fc1, fc2;
};
struct MhaW {           // AttnBlock / CrossAttnBlock (modules.py:133-204)
    LNw n1, n2, nctx;
    Lin in_proj;        // self: [3H, H]
    Lin q_proj, kv_proj;  // cross: rows [0:H] and [H:3H] of in_proj_weight
    Lin out_proj, fc1, fc2;
    bool cross = false;
};
struct TrackW {
    float* qrt = nullptr;    // query_ref_token [2, 3L+4]
    float* virt = nullptr;   // virual_tracks [V, Hh]
    Lin corr_fc1, corr_fc2, input_transform, flow_head, ffeat_updater, vis, conf;
    LNw input_norm, output_norm, fmap_norm, ffeat_norm;
    std::vector<MhaW> time, space_virtual, p2v, v2p;
};

struct Arena {
    char* base = nullptr;
    size_t off = 0, peak = 0, cap = 0;
    bool dry = false, overflow = false;
    void* alloc(size_t bytes) {
        off = align_up(off, 256);
        void* p = dry ? (void*)(uintptr_t)(0x1000 + off) : (void*)(base + off);
        off += bytes;
        if (off > peak) peak = off;
        if (!dry && off > cap) overflow = true;
        return p;
    }
    size_t mark() const { return off; }
    void release(size_t m) { off = m; }
};

struct UvTab { int w, h, C; float* tx; float* ty; };

// Per-shape constant tables (RoPE positions and cos/sin tables, the DPT heads' UV embeddings): immutable
// entries, built on first use and kept until the handle is destroyed, so that forwards of ANY shapes may be in
// flight on one handle at the same time.  Keyed by the frame size (H, W): the RoPE and UV tables do not depend on
// the number of frames at all, and the position table of F frames is a prefix of the table of more frames -- an
// entry serves every call of up to `frames` frames; a call with more builds a new entry of at least twice the
// capacity that SHARES the first entry's RoPE / UV tables, so a caller that varies its batch size holds at most
// 2 x the largest position table it ever asked for (the cache used to grow with every distinct F).
struct ShapeTabs {
    int frames = 0;                 // capacity of pos in frames
    int* pos = nullptr;             // int32 [frames*P, 2]
    float *rope_cos = nullptr, *rope_sin = nullptr;
    int rope_npos = 0;
    const float* dino_pos = nullptr;   // DINOv2 pos_embed of this frame size (the model's own or a registered resize)
    std::vector<UvTab> uv;
    std::vector<void*> owned;
    ~ShapeTabs() {
        for (void* p : owned) (void)hipFree(p);
    }
};

}  // namespace vggt
}  // namespace skimi

struct skimi_vggt {
    skimi_vggt_config cfg;
    std::map<std::string, std::pair<float*, int64_t>> raw;   // staged fp32 weights (device)
    std::vector<void*> owned;                                // packed device buffers
    bool finalized = false;
    bool dpt_oc1_coarse = true;   // SKIMI_DPT_OC1_COARSE (read at create): output_conv1 of the bf16x3 heads contracted before the x2 upsample
    bool dpt_fold = true;   // SKIMI_DPT_FOLD (read at create): fold the bf16x3 heads' ConvTranspose resizes into layer1_rn / layer2_rn
    // packed model
    skimi::vggt::Lin patch_proj;    // [C, Kp] patchify GEMM (K = 3*p*p padded to 8)
    int patch_kp = 0;
    float* dino_pos = nullptr;      // pos_embed [1 + np0, C]
    std::map<std::pair<int, int>, float*> dino_pos_alt;   // (H, W) -> resized pos_embed [1 + ph*pw, C]
    float* dino_special = nullptr;  // [2][1+R][C] (cls + pos[0], registers), both selector rows equal
    float* agg_special = nullptr;   // [2][1+R][C] camera/register tokens for frame 0 / others
    std::vector<skimi::vggt::BlockW> dino, frame, global;
    skimi::vggt::LNw dino_norm;
    skimi::vggt::CamW cam;
    skimi::vggt::DptW depth, point, trackf;
    skimi::vggt::TrackW track;
    // per-shape tables: keyed cache, entries immutable once published (prepare())
    std::mutex prep_mu;             // guards the map; the entries themselves are read-only
    std::map<std::pair<int, int>, std::vector<std::unique_ptr<skimi::vggt::ShapeTabs>>> tabs;   // (H, W) -> entries of growing frame capacity
};

namespace skimi {
namespace vggt {

// ------------------------------------------------------------------------------------------
// weight packer (vggt_pack.hip): staged fp32 weights -> the packed model, once, in skimi_vggt_finalize
// ------------------------------------------------------------------------------------------
struct Packer {
    skimi_vggt* h;
    int rc = SKIMI_OK;
    hipStream_t st = nullptr;

    float* raw(const std::string& key, int64_t n);
    void* dmalloc(size_t bytes);
    float* keep(const std::string& key, int64_t n);
    LNw ln(const std::string& p, int C) { return LNw{keep(p + ".weight", C), keep(p + ".bias", C)}; }
    Lin pack_matrix(float* src, int N, int K, int prec);
    Lin linear(const std::string& p, int N, int K, int prec, bool bias = true);
    Lin linear_named(const std::string& wkey, const std::string& bkey, int N, int K, int prec);
    void add_records(Lin& L);
    ConvW conv(const std::string& p, int Co, int Ci, int k, int stride, int pad, int prec, bool bias);
    Lin convT(const std::string& p, int C, int s, int prec);
    Lin conv_taps(const std::string& p, int Co, int Ci);
    Lin conv_fold(const std::string& pT, const std::string& pRn, int C, int Co, int s);
    void add_fp8(Lin& L, const std::string& p, int N, int K);
    BlockW block(const std::string& p, int C, int hidden, bool qk_norm, int hd, int prec_in);
    DptW dpt(const std::string& p, int D, int features, const int* oc, int n_out, bool feature_only, int prec);
};

// everything skimi_vggt_finalize packs (the handle's previous packed buffers already released); ends synchronised
int pack_model(skimi_vggt* h);
void pack_track(Packer& pk, skimi_vggt* h);   // vggt_track.hip

// ------------------------------------------------------------------------------------------
// forward context (vggt_block.hip)
// ------------------------------------------------------------------------------------------
struct Ctx {
    skimi_vggt* h;
    hipStream_t st;
    const ShapeTabs* tabs = nullptr;   // this call's shape tables (null in a dry run)
    Arena ar;
    int rc = SKIMI_OK;
    void* slab = nullptr;      // split-K scratch
    size_t slab_bytes = 0;

    bool dry() const { return ar.dry; }
    // operand format of the Linears' activations: fp32 (split hi + lo by the kernels), fp16, or bf16 (BF16 and FP8 modes)
    static int act_dt(int prec) { return prec == SKIMI_PREC_BF16X3 ? SKIMI_F32 : prec == SKIMI_PREC_F16 ? SKIMI_F16 : SKIMI_BF16; }
    static size_t esz(int dt) { return dt == SKIMI_F32 ? 4 : 2; }

    // THE launch guard: `launch` () -> SKIMI_* code runs unless an earlier step failed or this is the dry run that sizes
    // the workspace.  It takes a callable so that the launch's arguments stay unevaluated then: the dry run's pointers
    // are fake (0x1000 + offset) and it has no shape tables (tabs == nullptr).
    template <class Launch>
    void run(Launch&& launch) {
        if (!rc && !dry()) rc = launch();
    }
    // `d` reading its A operand as bf16x3 records ([K/32][hi 32 | lo 32] per row) at `rec`, `rec_bytes` of them with the
    // zero page right behind.  Eligibility probes pass a fake `rec`: gemm_x3dma_eligible looks at alignment and
    // distances only.
    static skimi_gemm_desc as_records(skimi_gemm_desc d, void* rec, size_t rec_bytes) {
        d.A = rec; d.a_dtype = SKIMI_BF16X3_REC;
        d.x3_scratch = (char*)rec + rec_bytes; d.x3_scratch_bytes = 256;
        return d;
    }

    void gemm(skimi_gemm_desc& d);
    skimi_gemm_desc desc(const Lin& L, const void* A, int a_dt, long lda, int M, void* out, int out_dt, long ldo);
    void conv_geom(skimi_gemm_desc& d, const ConvW& c, int N, int H, int W, int OH, int OW);
    void ln(const float* x, const float* x2, long ldx, long rows, int C, const LNw& w, float eps, void* out, int odt,
            long grp_rows = 0, long grp_stride = 0, long grp_off = 0);
    void copy(void* dst, const void* src, size_t bytes);
    void zero(void* dst, size_t bytes);
};

struct BlockBufs { void* xn; void* qkv; void* ao; void* hid; void* q8 = nullptr; void* q8s = nullptr; };   // q8: MXFP8 scratch [M][4C] + scales
struct MhaBufs { float *xn, *cn, *q, *kv, *ao, *hid; };   // scratch of one track-head AttnBlock / CrossAttnBlock

// ------------------------------------------------------------------------------------------
// the parts: each enqueues its launches on c.st, allocates from c.ar, and leaves its status in c.rc
// ------------------------------------------------------------------------------------------
void run_block(Ctx& c, const BlockW& w, float* x, int batch, int seq, int C, int heads, float eps, bool rope,
               const BlockBufs& b);                                                            // vggt_block.hip
void run_camera(Ctx& c, const CamW& w, const float* sf, const float* sg, int B, int S, int P, int C, float* out_list,
                float* out_last);                                                              // vggt_camera.hip
const UvTab* find_uv(const ShapeTabs* h, int w, int hh, int C);                                // vggt_dpt.hip
bool dpt_fused_ln(const DptW& w, int f2, int udt);
int dpt_oc1_coarse_count();   // heads on the calling thread whose output_conv1 ran on the coarse map so far (tests)
void* run_dpt(Ctx& c, const DptW& w, float* const* sf, float* const* sg, int F, int P, int nsp, int ph, int pw, int C,
              int H, int W, float* pts, float* conf, int act_mode);
void run_track(Ctx& c, float* const* sf, float* const* sg, int B, int S, int P, int nsp, int ph, int pw, int C, int H, int W,
               const float* query, int N, float* out_track, float* out_vis, float* out_conf);  // vggt_track.hip

}  // namespace vggt
}  // namespace skimi
