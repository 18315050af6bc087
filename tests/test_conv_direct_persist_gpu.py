"""The fused tail of the DPT heads (csrc/conv_direct.hip, conv_direct_n32_kernel<true>, ops.conv3x3_n32_upsampled): the
direct 3x3 -> 32 conv interpolates its window from the coarse fp32 map itself, walking the tiles in a persistent loop,
against the two launches it replaces (skimi_resize_bilinear_planes into pixel records + the one-tile-per-workgroup conv on
them), bit for bit.

Both compute every window value through the same helpers (vggt_kernels.h) and run the same MFMAs per output in the same
order, so the results must be equal; what the fused launch adds and can get wrong: the source window and UV rows it
stages per (tile, slice), zeros for halo pixels outside the image, which tile a workgroup takes next, the buffer parity
carried across tiles, the next tile's slice 0 staged under the last slice of this one, and stores still in flight when
the next tile starts.  With and without the UV tables; SKIMI_CONV_DIRECT_GRID caps the workgroups: 1 (one workgroup
walks every tile in order), 5 (the tile count is no multiple of the grid) and unset (more CUs than tiles: one tile
each).  The output is NaN-filled first and lies between NaN guard bands that must stay NaN.
(F, h x w -> H x W, C):
  (2, 10x12 -> 17x21, 64)   ragged tiles; the clamped last source row and column (y1 = x1 = the last sample); a workgroup's
                            walk crosses the frame seam
  (1, 19x19 -> 33x33, 96)   odd slice count: the parity flips from tile to tile; C / 2 = 48 splits slice 1 between tabx and taby
  (3, 9x9 -> 16x16, 32)     exact tile, one slice
  (1, 30x30 -> 33x33, 32)   a window touches more than 12 source samples: the two launches must run, and still agree
and one whole forward (the model of test_dpt_fold_gpu.py: real head channel counts on a small aggregator) with
SKIMI_DPT_TAIL_FUSED on and off, whose dense maps must be bit-identical."""
import contextlib
import functools
import os

import pytest
import torch

import conv_direct_restated as R
from skiing_analysis_pytorch_amd import ops, vggt, weights as W
from skiing_analysis_pytorch_amd._lib import PREC_BF16X3

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64
GRIDS = [1, 5, None]
SWITCHES = ("SKIMI_CONV_DIRECT_GRID", "SKIMI_DPT_TAIL_FUSED")   # re-read per launch: conftest sets SKIMI_ENV_DYNAMIC=1
UP_CASES = [(2, 10, 12, 17, 21, 64, True), (1, 19, 19, 33, 33, 96, True), (3, 9, 9, 16, 16, 32, True),
            (1, 30, 30, 33, 33, 32, False)]   # F, h, w, H, W, C, whether the one launch is eligible


@contextlib.contextmanager
def _switches(**kv):
    """the kernel switches set (None: unset) for the launches inside, whatever the caller's environment says"""
    saved = {k: os.environ.pop(k, None) for k in SWITCHES}
    try:
        os.environ.update({k: str(v) for k, v in kv.items() if v is not None})
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


@functools.lru_cache(maxsize=None)
def _up_case(case, tables):
    """(coarse map, tabx, taby, packed weight, bias, the two launches' guarded output on the CPU): made once per case"""
    F_, h, w, H, W_, C, _ = case
    g = R.gen(900 + UP_CASES.index(case))
    src = torch.randn(F_, h, w, C, generator=g).to(DEV)
    tabx = (0.1 * torch.randn(W_, C // 2, generator=g)).to(DEV) if tables else None
    taby = (0.1 * torch.randn(H, C // 2, generator=g)).to(DEV) if tables else None
    packed = ops.conv3x3_n32_pack((torch.randn(32, C, 3, 3, generator=g) / (9 * C) ** 0.5).to(DEV))
    b = torch.randn(32, generator=g).to(DEV)
    rec = torch.empty(F_, H, W_, 2 * C, dtype=torch.bfloat16, device=DEV)
    ov, obuf = R.guarded(torch.full((F_, H, W_, 32), float("nan")), GUARD, DEV)
    with _switches():
        ops.resize_bilinear_planes(src, H, W_, rec, tabx=tabx, taby=taby, records=False)
        ops.conv3x3_n32((F_, H, W_, C), None, b, True, planes=(rec, rec.view(-1)[C:]), px_stride=2 * C, packed=packed, out=ov)
        torch.cuda.synchronize()
    want = obuf.cpu()
    assert (rec[..., C:].float() != 0).float().mean() > 0.5, "the lo halves must carry value"
    return src, tabx, taby, packed, b, want


@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: f"grid{g}")
@pytest.mark.parametrize("tables", [True, False], ids=["uv", "nouv"])
@pytest.mark.parametrize("case", UP_CASES, ids=lambda c: "x".join(map(str, c[:6])))
def test_fused_upsample_is_bit_identical(case, tables, grid):
    F_, h, w, H, W_, C, eligible = case
    src, tabx, taby, packed, b, want = _up_case(case, tables)
    n = GUARD * 32
    assert torch.isnan(want[:n]).all() and torch.isnan(want[-n:]).all() and not torch.isnan(want[n:-n]).any()
    for switch, ran in ((None, eligible), (0, False)):
        ov, obuf = R.guarded(torch.full((F_, H, W_, 32), float("nan")), GUARD, DEV)
        with _switches(SKIMI_CONV_DIRECT_GRID=grid, SKIMI_DPT_TAIL_FUSED=switch):
            _, fused = ops.conv3x3_n32_upsampled(src, H, W_, packed, b, True, tabx=tabx, taby=taby, out=ov)
            torch.cuda.synchronize()
        assert fused == ran, f"SKIMI_DPT_TAIL_FUSED={switch}: the {'one launch' if fused else 'two launches'} ran"
        got = obuf.cpu()
        assert torch.isnan(got[:n]).all() and torch.isnan(got[-n:]).all(), "elements outside the output were written"
        diff = got[n:-n].view(torch.int32) != want[n:-n].view(torch.int32)
        assert not diff.any(), f"fused={fused}: {int(diff.sum())} of {diff.numel()} elements differ; first at pixel " \
                               f"{int(diff.nonzero()[0]) // 32} of {F_} x {H} x {W_}"


def test_whole_head_tail_fused_on_vs_off():
    """depth and point heads at their real channel counts (the tail runs 128 -> 32 on an 80 x 80 -> 140 x 140 resize with the
    UV tables): every dense map bit-identical with the switch on and off"""
    cfg = W.VGGTConfig(img_size=140, embed_dim=256, depth=4, num_heads=4, patch_embed="conv", cam_trunk_depth=2, cam_heads=8,
                       dpt_features=256, dpt_out_channels=(256, 512, 1024, 1024), dpt_layers=(0, 1, 2, 3), track_features=64,
                       track_hidden=128, track_corr_levels=3, track_corr_radius=3, track_iters=3, track_depth=2, track_heads=8,
                       track_virtual=16)
    sd = W.make_vggt_state_dict(cfg, seed=0, device=DEV)
    images = W.make_images(3, 140, 140, seed=7)[None].to(DEV)
    m = vggt.VGGT(config=cfg, prec=PREC_BF16X3, head_prec=PREC_BF16X3)
    m.load_state_dict(sd)
    outs = {}
    for switch in (1, 0):
        with _switches(SKIMI_DPT_TAIL_FUSED=switch):
            out = m(images, want={"depth", "point"})
            torch.cuda.synchronize()
        outs[switch] = {k: out[k].clone() for k in ("depth", "depth_conf", "world_points", "world_points_conf")}
    for k, a in outs[1].items():
        assert torch.isfinite(a).all(), k
        assert torch.equal(a.view(torch.int32), outs[0][k].view(torch.int32)), \
            f"{k}: {int((a != outs[0][k]).sum())} of {a.numel()} elements differ"
