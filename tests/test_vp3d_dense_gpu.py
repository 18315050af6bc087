"""GPU: TemporalModel(dense=True) (model.py:113-116) through the C-ABI against the reference's own dense outputs
(tests/golden/vp3d_*_dense.npz) and the float64 restatement tests/vp3d_dense_restated.py: the small-batch streaming
path with the tap-reuse window kernel (csrc/vp3d_dense.hip) for the wide convs, the per-tap kernel it replaces,
the generic GEMM chain of large batches, bf16 mode and the reference-signature entry point."""
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import vp3d_dense_restated as R  # noqa: E402

from oracle import vp3d_oracle  # noqa: E402
from skiing_analysis_pytorch_amd import run as vp_run, vp3d, weights as W  # noqa: E402
from skiing_analysis_pytorch_amd._lib import PREC_BF16, PREC_BF16X3  # noqa: E402

pytestmark = pytest.mark.gpu

TOL_JOINTS = 1e-3   # as test_vp3d_matches_reference_golden


def _model(fw, causal=False, prec=PREC_BF16X3, seed=0):
    sd = W.make_vp3d_state_dict(seed=seed, filter_widths=fw, dense=True)
    m = vp3d.TemporalModel(17, 2, 17, fw, causal=causal, channels=1024, dense=True, prec=prec)
    m.load_state_dict(sd)
    return m, sd


@pytest.mark.parametrize("name", ["rf27_dense", "rf27_dense_causal", "rf243_dense", "w535_dense"])
def test_vp3d_dense_matches_reference_golden(golden_dir, name):
    g = np.load(golden_dir / f"vp3d_{name}.npz")
    fw = [int(v) for v in g["filter_widths"]]
    causal = bool(g["causal"])
    m, _ = _model(fw, causal)
    assert m.dense and m.receptive_field() == int(g["receptive_field"])
    for aug in (0, 1):
        x = torch.from_numpy(g[f"batch2d_aug{aug}"]).cuda()
        raw = m(x).cpu().numpy()
        assert raw.shape == g[f"raw_aug{aug}"].shape
        err = np.abs(raw - g[f"raw_aug{aug}"]).max()
        assert err < 2e-4, f"{name} aug{aug}: max abs err {err}"
        pred = vp3d.lift_clip(m, g["keypoints_px"], int(g["w"]), int(g["h"]), augment=bool(aug))
        mp = vp3d_oracle.mpjpe(pred, g[f"pred_aug{aug}"])
        assert mp < TOL_JOINTS and np.abs(pred - g[f"pred_aug{aug}"]).max() < TOL_JOINTS


@pytest.mark.parametrize("fw", [[3, 3, 3], [3, 5, 3]])
def test_vp3d_dense_other_seed(fw):
    m, sd = _model(fw, seed=5)
    for frames in (1, 27, 100):        # ragged clip lengths incl. a single output frame
        kp = W.make_keypoints_2d(frames=frames, seed=9).numpy()
        ref = R.lift_clip(sd, kp, 1920, 1080, fw)
        out = vp3d.lift_clip(m, kp, 1920, 1080)
        assert out.shape == (frames, 17, 3)
        assert np.abs(out - ref).max() < 2e-4


@pytest.mark.parametrize("fw,causal", [([3, 3, 3], False), ([3, 3, 3], True), ([3, 5, 3], False)])
def test_vp3d_dense_small_batches_on_the_streaming_path(fw, causal):
    """B = 1 .. 6: every clip equals its single-clip run and the restatement; no atomics, two runs bit-identical."""
    m, sd = _model(fw, causal)
    rf = m.receptive_field()
    for B, frames in ((1, rf), (1, rf + 242), (2, rf + 242), (2, rf + 57), (3, rf + 100), (4, rf + 242), (5, rf + 17),
                      (6, rf + 130)):
        x = torch.randn(B, frames, 17, 2, device="cuda", generator=torch.Generator(device="cuda").manual_seed(B * 7 + frames))
        out = m(x)
        assert out.shape == (B, frames - rf + 1, 17, 3)
        assert torch.equal(out, m(x))
        with torch.no_grad():
            ref = R.forward(sd, x.cpu(), fw, causal)
        assert (out.cpu().double() - ref).abs().max().item() < 2e-4 * max(1.0, ref.abs().max().item())
        for i in range(B):
            one = m(x[i:i + 1].contiguous())
            assert (out[i] - one[0]).abs().max().item() < 1e-5 * max(1.0, one.abs().max().item())


def test_vp3d_dense_window_kernel_matches_per_tap_kernel(monkeypatch):
    """The window kernel against the per-tap kernel it replaces (SKIMI_VP3D_WINDOW=0, re-read per forward under the
    suite's SKIMI_ENV_DYNAMIC=1): the same bf16x3 products summed in another order.  RF 243: 7, 19, 55 and 163 taps."""
    fw = [3, 3, 3, 3, 3]
    m, sd = _model(fw)
    rf = m.receptive_field()
    x = torch.randn(2, rf + 242, 17, 2, device="cuda", generator=torch.Generator(device="cuda").manual_seed(11))
    monkeypatch.setenv("SKIMI_VP3D_WINDOW", "1")
    win = m(x)
    monkeypatch.setenv("SKIMI_VP3D_WINDOW", "0")
    tap = m(x)
    monkeypatch.setenv("SKIMI_VP3D_WINDOW", "1")
    with torch.no_grad():
        ref = R.forward(sd, x.cpu(), fw)
    scale = max(1.0, ref.abs().max().item())
    assert (win.cpu().double() - ref).abs().max().item() < 2e-4 * scale
    assert (tap.cpu().double() - ref).abs().max().item() < 2e-4 * scale
    assert (win - tap).abs().max().item() < 2e-5 * scale


def test_vp3d_dense_large_batch():
    """Past the streaming threshold (2048 rows of the first layer) the generic GEMM chain runs the wide convs."""
    fw = [3, 3, 3]
    m, sd = _model(fw)
    rf = m.receptive_field()
    frames = rf + 242
    x = torch.randn(8, frames, 17, 2, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    assert 8 * (frames - 2) > 2048
    big = m(x)
    with torch.no_grad():
        ref = R.forward(sd, x.cpu(), fw)
    assert (big.cpu().double() - ref).abs().max().item() < 2e-4 * max(1.0, ref.abs().max().item())
    for i in (0, 5):
        one = m(x[i:i + 1].contiguous())
        assert (big[i] - one[0]).abs().max().item() < 5e-5 * one[0].abs().max().item()


def test_vp3d_dense_bf16_mode_tolerance():
    fw = [3, 3, 3]
    m, sd = _model(fw, prec=PREC_BF16)
    kp = W.make_keypoints_2d(frames=243, seed=1).numpy()
    ref = R.lift_clip(sd, kp, 1920, 1080, fw)
    out = vp3d.lift_clip(m, kp, 1920, 1080)
    rel = np.linalg.norm(out - ref) / np.linalg.norm(ref)
    assert rel < 3e-2, rel


@pytest.mark.parametrize("tta", [True, False])
def test_run_video_pose_3d_dense(tmp_path, tta):
    """run.run_video_pose_3d with the reference's own --dense flag, a `{"model_pos": sd}` checkpoint and a .pt clip."""
    arch, fw = "3,3,3", [3, 3, 3]
    sd = W.make_vp3d_state_dict(seed=0, filter_widths=fw, dense=True)
    torch.save({"epoch": 80, "model_pos": sd}, tmp_path / "ckpt.bin")
    T, H, Wd = 50, 1080, 1920
    kp = W.make_keypoints_2d(frames=T, seed=2)
    torch.save({"video_name": "run01", "video_path": "/videos/run01.mp4", "img_shape": (H, Wd),
                "detectron2": {"keypoints": kp, "bbox": torch.zeros(T, 4)}, "depth": torch.rand(T, 1, 6, 8)},
               tmp_path / "run01.pt")
    args = SimpleNamespace(architecture=arch, causal=False, dropout=0.25, channels=1024, dense=True, test_time_augmentation=tta)
    config = {"model": {"ckpt_path": str(tmp_path / "ckpt.bin")}}
    pred, _ = vp_run.run_video_pose_3d(config, tmp_path / "run01.pt", tmp_path / "vp3d_out", args)
    saved = np.load(tmp_path / "vp3d_out" / "run01.npy")
    assert saved.shape == (T, 17, 3)
    ref = R.lift_clip(sd, kp.numpy(), Wd, H, fw, augment=tta)
    assert np.abs(saved - ref).max() < 1e-3
    assert pred.shape == (T, 17, 3) and np.isfinite(pred).all()


def test_vp3d_dense_rejects_dilated_weights():
    fw = [3, 3, 3]
    m = vp3d.TemporalModel(17, 2, 17, fw, dense=True)
    with pytest.raises(RuntimeError, match="size mismatch for layers_conv.0.weight"):
        m.load_state_dict(W.make_vp3d_state_dict(seed=0, filter_widths=fw))
    # a dense checkpoint in a dilated model, and through the entry point's loader
    with pytest.raises(RuntimeError, match="size mismatch"):
        vp3d.TemporalModel(17, 2, 17, fw).load_state_dict(W.make_vp3d_state_dict(seed=0, filter_widths=fw, dense=True))
