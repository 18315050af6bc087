"""GPU: scratch.output_conv1 of the fp32-accurate DPT heads contracted on refinenet1's coarse map (dpt_head.py:447-455
then :287; run_dpt's SKIMI_DPT_OC1_COARSE path in vggt_dpt.hip): the conv's nine taps as ONE plain-row GEMM
[pixels x C] . [C x 9 C/2] on the LDS-DMA bf16x3 kernel, then dpt_tap_sum_kernel (vggt_kernels.hip), which resizes every
tap's result x2 (align-corners bilinear), shifts it by its tap and sums under the conv's zero-padding mask.

The reference is torch on the CPU in float64: conv2d(interpolate(x, scale 2, bilinear, align_corners=True), W, b, padding=1).
The fine path is what SKIMI_DPT_OC1_COARSE=0 launches: the resize into bf16x3 records, then the 3x3 conv as a slice-major
gather GEMM on the 128-column LDS-DMA kernel.  Channel counts are the real ones (256 -> 128); the coarse maps are 5 x 7
with 8 frames (280 rows: one full 256-row tile + a partial one), 21 x 37 with 3 frames (the 294 x 518 configuration) and
2 x 3 with 2 frames (every pixel a border pixel; 12 and 48 rows are below the LDS-DMA kernels' 256, so both paths' GEMMs
run on the generic bf16x3 kernel there, as the forward's would).  The fine sizes 10 x 14, 42 x 74 and 4 x 6 divide no tile
of the tap-sum kernel (16 x 32).

"Relative error" of an array = max |got - ref| / max |ref|.  Measured values: profiles/r08_summary.md."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from skiing_analysis_pytorch_amd import _lib, ops, vggt, weights as W
from skiing_analysis_pytorch_amd._lib import PREC_BF16X3

pytestmark = pytest.mark.gpu
DEV = "cuda"
CI, CO = 256, 128
MAPS = {"5x7": (8, 5, 7), "21x37": (3, 21, 37), "2x3": (2, 2, 3)}        # frames, h, w of the coarse map


def _reference(x, w, b):
    """float64 on the CPU; x [F, h, w, Ci] channels-last -> [F, 2h, 2w, Co]"""
    up = F.interpolate(x.double().permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=True)
    return F.conv2d(up, w.double(), b.double(), padding=1).permute(0, 2, 3, 1).contiguous()


def _records(x2d):
    rows, Cc = x2d.shape
    ar = ops.records_buffer(rows, Cc, device=x2d.device)
    ar[:rows * Cc * 2] = ops.split_records(x2d.contiguous()).reshape(-1)
    ar[rows * Cc * 2:] = 0
    return ar


def _fine(x, w, b):
    """the launches of SKIMI_DPT_OC1_COARSE=0 (run_dpt's r == 0 branch and the prev_rec launch below it)"""
    Fr, h, w_, Ci = x.shape
    Co = w.shape[0]
    H, W_ = 2 * h, 2 * w_
    M = Fr * H * W_
    wsl = w.permute(0, 2, 3, 1).reshape(Co, 3, 3, Ci // 32, 32).permute(0, 3, 1, 2, 4).reshape(Co, 9 * Ci).contiguous()
    conv = dict(N=Fr, H=H, W=W_, C=Ci, KH=3, KW=3, stride=1, pad=1, dil=1, OH=H, OW=W_, slice_major=True)
    if M >= 256:
        rec = ops.records_buffer(M, Ci)
        ops.resize_bilinear_planes(x, H, W_, rec, records=True, zpage=rec[M * Ci * 2:])
        o = ops.gemm(None, wsl, prec=PREC_BF16X3, conv=conv, bias=b, a_records=rec, w_split=ops.split_records(wsl))
        assert ops.gemm_last_path().family == "x3dma_narrow"
    else:       # below the 256-row kernels: fp32 resize + the generic bf16x3 kernel
        up = ops.resize_bilinear(x, H, W_)
        o = ops.gemm(up.view(M, Ci), wsl, prec=PREC_BF16X3, conv=conv, bias=b)
        assert ops.gemm_last_path().family == "generic"
    return o.view(Fr, H, W_, Co)


def _coarse(x, w, b):
    """the launches of SKIMI_DPT_OC1_COARSE=1: the nine taps contracted on the coarse map, then the tap sum"""
    Fr, h, w_, Ci = x.shape
    Co = w.shape[0]
    M = Fr * h * w_
    w9 = ops.conv3x3_taps_matrix(w)
    if M >= 256:
        taps = ops.gemm(None, w9, prec=PREC_BF16X3, a_records=_records(x.reshape(M, Ci)), M=M, lda=Ci, w_split=ops.split_records(w9))
        assert ops.gemm_last_path().family == "x3dma_wide"
    else:
        taps = ops.gemm(x.reshape(M, Ci), w9, prec=PREC_BF16X3)
        assert ops.gemm_last_path().family == "generic"
    return ops.dpt_tap_sum(taps.view(Fr, h, w_, 9, Co), b)


def _rel(got, ref):
    return float((got.double().cpu() - ref).abs().max() / ref.abs().max())


def _check(x, w, b, what):
    """coarse path's error against float64 <= 2 x the fine path's on the same inputs (2 = margin for the changed fp32
    summation order, the rule of the ConvTranspose fold's test)"""
    ref = _reference(x, w, b)
    dev = [t.to(DEV) for t in (x, w, b)]
    coarse, fine = _coarse(*dev), _fine(*dev)
    torch.cuda.synchronize()
    e_c, e_f = _rel(coarse, ref), _rel(fine, ref)
    print(f"{what}: coarse {e_c:.3e}  fine {e_f:.3e}  (max |got - float64| / max |float64|)")
    assert np.isfinite(e_c) and e_c <= 2.0 * e_f, (e_c, e_f)


@pytest.mark.parametrize("fmap", list(MAPS))
def test_coarse_no_worse_than_fine_against_float64(fmap, monkeypatch):
    monkeypatch.setenv("SKIMI_X3_MIN_TILES", "1")
    Fr, h, w_ = MAPS[fmap]
    g = torch.Generator().manual_seed(len(fmap) + 7 * h)
    x = torch.randn((Fr, h, w_, CI), generator=g)
    w = torch.randn((CO, CI, 3, 3), generator=g) / (9 * CI) ** 0.5
    b = torch.randn((CO,), generator=g)
    _check(x, w, b, f"map {fmap}")


@pytest.mark.parametrize("fmap", ["5x7", "2x3"])
def test_bias_and_padding_mask_on_ones(fmap, monkeypatch):
    """input of all ones: every output is bias + the sum of the taps that stay inside the map (the resize of a constant is
    the constant), so only the bias and the padding mask decide"""
    monkeypatch.setenv("SKIMI_X3_MIN_TILES", "1")
    Fr, h, w_ = MAPS[fmap]
    g = torch.Generator().manual_seed(41)
    x = torch.ones((Fr, h, w_, CI))
    w = torch.randn((CO, CI, 3, 3), generator=g) / (9 * CI) ** 0.5
    b = torch.randn((CO,), generator=g)
    _check(x, w, b, f"ones, map {fmap}")


@pytest.mark.parametrize("tap", range(9))
def test_single_tap(tap, monkeypatch):
    """bias = 0 and one non-zero tap: a transposed or mirrored tap index moves the whole map by a pixel"""
    monkeypatch.setenv("SKIMI_X3_MIN_TILES", "1")
    Fr, h, w_ = MAPS["5x7"]
    g = torch.Generator().manual_seed(50 + tap)
    x = torch.randn((Fr, h, w_, CI), generator=g)
    w = torch.zeros((CO, CI, 3, 3))
    w[:, :, tap // 3, tap % 3] = torch.randn((CO, CI), generator=g) / CI ** 0.5
    _check(x, w, torch.zeros((CO,)), f"tap {tap}")


def test_whole_head_coarse_on_vs_off(monkeypatch):
    """a full forward (real DPT channel counts on a small aggregator) with SKIMI_DPT_OC1_COARSE=1 vs 0: the dense maps agree to
    fp32 rounding level -- bounded by the heads' 1e-3 parity tolerance against the oracle, which both settings must meet --
    and cameras and tracks, which do not read these maps, are bit-identical.  The library counts the heads that took the
    coarse path (both with =1, none with =0: a silent fallback fails here), and the forward's sizing pass and its real pass
    take the same bytes from the workspace."""
    monkeypatch.setenv("SKIMI_X3_MIN_TILES", "1")
    cfg = W.VGGTConfig(img_size=140, embed_dim=256, depth=4, num_heads=4, patch_embed="conv", cam_trunk_depth=2, cam_heads=8,
                       dpt_features=256, dpt_out_channels=(256, 512, 1024, 1024), dpt_layers=(0, 1, 2, 3), track_features=64,
                       track_hidden=128, track_corr_levels=3, track_corr_radius=3, track_iters=3, track_depth=2, track_heads=8,
                       track_virtual=16)
    sd = W.make_vggt_state_dict(cfg, seed=0, device=DEV)
    images = W.make_images(3, 140, 140, seed=7)[None].to(DEV)
    queries = (torch.rand((1, 5, 2), generator=torch.Generator().manual_seed(3)) * 100 + 20).to(DEV)
    outs, took = {}, {}
    lib = _lib.lib()
    for sw in ("1", "0"):
        monkeypatch.setenv("SKIMI_DPT_OC1_COARSE", sw)     # read when the handle is created
        m = vggt.VGGT(config=cfg, prec=PREC_BF16X3, head_prec=PREC_BF16X3)
        m.load_state_dict(sd)
        before = lib.skimi_vggt_oc1_coarse_count()
        out = m(images, query_points=queries)
        torch.cuda.synchronize()
        took[sw] = lib.skimi_vggt_oc1_coarse_count() - before
        planned, used = C.c_uint64(0), C.c_uint64(0)
        assert lib.skimi_vggt_last_arena(C.byref(planned), C.byref(used)) == 0
        print(f"SKIMI_DPT_OC1_COARSE={sw}: heads on the coarse path {took[sw]}, workspace planned {planned.value} used {used.value}")
        assert planned.value == used.value > 0, (sw, planned.value, used.value)
        outs[sw] = {k: (torch.stack(v) if isinstance(v, list) else v).clone() for k, v in out.items()}
        del m
    assert took == {"1": 2, "0": 0}, took
    for k in ("pose_enc", "pose_enc_list", "track", "vis", "conf"):
        assert torch.equal(outs["1"][k], outs["0"][k]), k
    differs = False
    for k in ("depth", "depth_conf", "world_points", "world_points_conf"):
        a, b = outs["1"][k].double(), outs["0"][k].double()
        d, scale = float((a - b).abs().max()), float(b.abs().max())
        print(f"{k}: max abs difference {d:.3e}, relative to max abs value {d / scale:.3e}")
        assert np.isfinite(d) and d / scale < 1e-3, (k, d, scale)
        differs |= d > 0
    assert differs, "SKIMI_DPT_OC1_COARSE=1 gave the same bits as =0"
