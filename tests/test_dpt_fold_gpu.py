"""GPU: the DPT heads' ConvTranspose resize folded into the following 3x3 layer_rn conv (levels 0 and 1 of
dpt_head.py:218-221, 273-274; gemm_x3w4_kernel<3> in gemm_x3dma.hip, weights by skimi_dpt_fold_pack).

The reference is torch on the CPU in float64: conv2d(conv_transpose2d(x, W_T, b_T, stride = s), W_rn, padding = 1).
The unfolded path is what SKIMI_DPT_FOLD=0 launches: the ConvTranspose as a pixel-shuffle GEMM, then the 3x3 conv as a
slice-major gather GEMM, both on the LDS-DMA bf16x3 kernels.  Channel counts are the real ones (level 0: 256 -> 256 -> 256,
s = 4; level 1: 512 -> 512 -> 256, s = 2); the maps are small (5 x 7: every border class and every phase occurs, and
8 frames are 280 rows = one full 256-row tile + a partial one) and 21 x 37 (the 294 x 518 configuration, ph != pw, 3 frames
= 2331 rows, not a multiple of the tile).

"Relative error" of an array here = max |got - ref| / max |ref| (the element-wise quotient has no meaning where the
reference passes through zero).  Measured values: profiles/r06_summary.md.

The tiny golden models (tests/golden/vggt_tiny_*) have 128 / 64 DPT features: below the 256-column kernel the folded form
runs on, so they keep the unfolded path; the cases here cover the folded one at the real channel counts instead."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from skiing_analysis_pytorch_amd import ops, vggt, weights as W
from skiing_analysis_pytorch_amd._lib import ACT_NONE, ACT_RELU, PREC_BF16X3

pytestmark = pytest.mark.gpu
DEV = "cuda"
LEVELS = {0: (256, 256, 4), 1: (512, 256, 2)}          # level -> (C of the ConvTranspose, features, stride)
MAPS = {"5x7": (8, 5, 7), "21x37": (3, 21, 37)}        # frames, h, w of the coarse map
CASES = [(lvl, m) for lvl in LEVELS for m in MAPS]


def _reference(x, wT, bT, wrn, s):
    """float64 on the CPU; x [F, h, w, C] channels-last -> [F, s h, s w, Co]"""
    u = F.conv_transpose2d(x.double().permute(0, 3, 1, 2), wT.double(), bT.double(), stride=s)
    return F.conv2d(u, wrn.double(), padding=1).permute(0, 2, 3, 1).contiguous()


def _unfolded(x, wT, bT, wrn, s, act):
    """the launches of SKIMI_DPT_FOLD=0 (Packer::convT + Packer::conv in vggt_pack.hip, run_dpt in vggt_dpt.hip)"""
    Fr, h, w, C = x.shape
    Co = wrn.shape[0]
    wps = wT.permute(2, 3, 1, 0).reshape(s * s * C, C).contiguous()               # [(a, b, co), ci]
    xa = x.reshape(-1, C).contiguous()
    u = ops.gemm(xa, wps, prec=PREC_BF16X3, bias=bT.repeat(s * s), pixel_shuffle=(s, C, Fr, h, w),
                 w_split=ops.split_records(wps), x3_scratch=torch.empty(ops.x3_scratch_numel(*xa.shape), device=DEV))
    assert ops.gemm_last_path().family == "x3dma_wide"
    M = Fr * h * s * w * s
    wsl = wrn.permute(0, 2, 3, 1).reshape(Co, 3, 3, C // 32, 32).permute(0, 3, 1, 2, 4).reshape(Co, 9 * C).contiguous()
    conv = dict(N=Fr, H=h * s, W=w * s, C=C, KH=3, KW=3, stride=1, pad=1, dil=1, OH=h * s, OW=w * s, slice_major=True)
    o = ops.gemm(u.reshape(M, C), wsl, prec=PREC_BF16X3, conv=conv, act=act, w_split=ops.split_records(wsl),
                 x3_scratch=torch.empty(ops.x3_scratch_numel(M, C), device=DEV))
    assert ops.gemm_last_path().family == "x3dma_wide"
    return o.view(Fr, h * s, w * s, Co)


def _folded(x, wT, bT, wrn, s, act, **kw):
    rec, beta = ops.dpt_fold_pack(wT, bT, wrn)
    o = ops.convT_conv3x3_folded(x, rec, beta, s, wrn.shape[0], act=act, **kw)
    assert ops.gemm_last_path().family == "x3dma_wide"
    return o


def _rel(got, ref):
    return float((got.double().cpu() - ref).abs().max() / ref.abs().max())


@pytest.mark.parametrize("level,fmap", CASES)
def test_folded_no_worse_than_unfolded_against_float64(level, fmap, monkeypatch):
    """random weights: the folded launch's error against float64 <= 2 x the unfolded path's on the same inputs (2 = margin for
    summation-order luck; folding removes one fp32 rounding of a whole map, so it is expected to hold with room)"""
    monkeypatch.setenv("SKIMI_X3_MIN_TILES", "1")
    C, Co, s = LEVELS[level]
    Fr, h, w = MAPS[fmap]
    g = torch.Generator().manual_seed(10 * level + len(fmap))
    x = torch.randn((Fr, h, w, C), generator=g)
    wT = torch.randn((C, C, s, s), generator=g) / C ** 0.5
    bT = torch.randn((C,), generator=g)
    wrn = torch.randn((Co, C, 3, 3), generator=g) / (9 * C) ** 0.5
    ref = _reference(x, wT, bT, wrn, s)
    dev = [t.to(DEV) for t in (x, wT, bT, wrn)]
    e_fold = _rel(_folded(*dev, s, ACT_NONE), ref)
    e_unf = _rel(_unfolded(*dev, s, ACT_NONE), ref)
    print(f"level {level} map {fmap}: folded {e_fold:.3e}  unfolded {e_unf:.3e}  (max |got - float64| / max |float64|)")
    assert e_fold <= 2.0 * e_unf, (e_fold, e_unf)


@pytest.mark.parametrize("level,fmap", CASES)
def test_folded_bit_identical_on_exact_integers(level, fmap, monkeypatch):
    """small-integer operands (every product, composite weight and partial sum exact in fp32 and in bf16 hi + lo): folded
    == unfolded == float64, bit for bit, borders included -- taps, phases, zero page and bias classes without a tolerance;
    the records written next to the fp32 rows are the split of those rows"""
    monkeypatch.setenv("SKIMI_X3_MIN_TILES", "1")
    C, Co, s = LEVELS[level]
    Fr, h, w = MAPS[fmap]
    g = torch.Generator().manual_seed(100 + 10 * level + len(fmap))
    ints = lambda shape, lim: torch.randint(-lim, lim + 1, shape, generator=g).float()
    x, wT, bT, wrn = ints((Fr, h, w, C), 3), ints((C, C, s, s), 1), ints((C,), 8), ints((Co, C, 3, 3), 2)
    ref = _reference(x, wT, bT, wrn, s).clamp_min(0)
    assert float(ref.abs().max()) < 2 ** 22          # far inside fp32's exact integers, partial sums too
    dev = [t.to(DEV) for t in (x, wT, bT, wrn)]
    M = Fr * h * s * w * s
    orec = ops.records_buffer(M, Co)
    orec.fill_(1.0)
    fold = _folded(*dev, s, ACT_RELU, out_records=orec)
    unf = _unfolded(*dev, s, ACT_RELU)
    torch.cuda.synchronize()
    assert torch.equal(fold, unf), int((fold != unf).sum())
    assert torch.equal(fold.double().cpu(), ref), float((fold.double().cpu() - ref).abs().max())
    assert torch.equal(orec[:M * Co * 2], ops.split_records(fold.view(M, Co)).reshape(-1))
    assert not orec[M * Co * 2:].any()               # the zero page behind the records
    only = ops.records_buffer(M, Co)
    assert _folded(*dev, s, ACT_RELU, out_records=only, records_only=True) is None
    assert torch.equal(only, orec)


def test_whole_head_fold_on_vs_off(monkeypatch):
    """a full forward (real DPT channel counts on a small aggregator) with SKIMI_DPT_FOLD=1 vs 0: the dense maps agree to
    fp32 rounding level -- bounded by the heads' 1e-3 parity tolerance against the oracle, which both settings must
    meet -- and joints' inputs (cameras) and tracks, which do not read these maps, are bit-identical"""
    monkeypatch.setenv("SKIMI_X3_MIN_TILES", "1")
    cfg = W.VGGTConfig(img_size=140, embed_dim=256, depth=4, num_heads=4, patch_embed="conv", cam_trunk_depth=2, cam_heads=8,
                       dpt_features=256, dpt_out_channels=(256, 512, 1024, 1024), dpt_layers=(0, 1, 2, 3), track_features=64,
                       track_hidden=128, track_corr_levels=3, track_corr_radius=3, track_iters=3, track_depth=2, track_heads=8,
                       track_virtual=16)
    sd = W.make_vggt_state_dict(cfg, seed=0, device=DEV)
    images = W.make_images(3, 140, 140, seed=7)[None].to(DEV)
    queries = (torch.rand((1, 5, 2), generator=torch.Generator().manual_seed(3)) * 100 + 20).to(DEV)
    outs = {}
    for fold in ("1", "0"):
        monkeypatch.setenv("SKIMI_DPT_FOLD", fold)     # read when the handle is created
        m = vggt.VGGT(config=cfg, prec=PREC_BF16X3, head_prec=PREC_BF16X3)
        m.load_state_dict(sd)
        out = m(images, query_points=queries)
        torch.cuda.synchronize()
        outs[fold] = {k: (torch.stack(v) if isinstance(v, list) else v).clone() for k, v in out.items()}
        del m
    for k in ("pose_enc", "pose_enc_list", "track", "vis", "conf"):
        assert torch.equal(outs["1"][k], outs["0"][k]), k
    differs = False
    for k in ("depth", "depth_conf", "world_points", "world_points_conf"):
        a, b = outs["1"][k].double(), outs["0"][k].double()
        d, scale = float((a - b).abs().max()), float(b.abs().max())
        print(f"{k}: max abs difference {d:.3e}, relative to max abs value {d / scale:.3e}")
        assert np.isfinite(d) and d / scale < 1e-3, (k, d, scale)
        differs |= d > 0
    assert differs, "SKIMI_DPT_FOLD=1 gave the same bits as =0: the folded launches did not run"
