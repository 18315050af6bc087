"""CPU: TemporalModel(dense=True) without a device -- the float64 restatement (tests/vp3d_dense_restated.py) against the
reference's own dense outputs (tests/golden/vp3d_*_dense.npz), the weight spec against the shapes the reference's
model holds, the dilated spec unchanged, the handle and the weight-shape check of the binding, and the tap-reuse
window kernel (csrc/vp3d_dense.hip) in the ISA the build's own flags emit."""
import re
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import vp3d_dense_restated as R  # noqa: E402

from skiing_analysis_pytorch_amd import weights as W  # noqa: E402

GOLDENS = ["rf27_dense", "rf27_dense_causal", "rf243_dense", "w535_dense"]


@pytest.mark.parametrize("name", GOLDENS)
def test_restatement_matches_dense_golden(golden_dir, name):
    g = np.load(golden_dir / f"vp3d_{name}.npz")
    fw = [int(v) for v in g["filter_widths"]]
    causal = bool(g["causal"])
    assert bool(g["dense"]) and R.receptive_field(fw) == int(g["receptive_field"])
    sd = W.make_vp3d_state_dict(seed=int(g["seed"]), filter_widths=fw, dense=True)
    for aug in (0, 1):
        with torch.no_grad():
            raw = R.forward(sd, torch.from_numpy(g[f"batch2d_aug{aug}"]), fw, causal).numpy()
        assert raw.shape == g[f"raw_aug{aug}"].shape
        # 1e-5 relative to the output's scale (~12 at RF 243): the golden is the reference's fp32 forward, whose sums
        # run over up to 163 x 1024 terms (8.8e-5 absolute at RF 243, below 1e-5 at the others)
        scale = max(1.0, float(np.abs(g[f"raw_aug{aug}"]).max()))
        assert np.abs(raw - g[f"raw_aug{aug}"]).max() < 1e-5 * scale, name
        with torch.no_grad():
            pred = R.lift_clip(sd, g["keypoints_px"], int(g["w"]), int(g["h"]), fw, causal, augment=bool(aug))
        assert np.abs(pred - g[f"pred_aug{aug}"]).max() < 1e-5 * scale, name


@pytest.mark.parametrize("name", GOLDENS)
def test_dense_spec_has_the_reference_shapes(golden_dir, name):
    g = np.load(golden_dir / f"vp3d_{name}.npz")
    fw = [int(v) for v in g["filter_widths"]]
    spec = W.vp3d_spec(filter_widths=fw, dense=True)
    for key, shape in zip(g["conv_weight_keys"], g["conv_weight_shapes"]):
        assert tuple(spec[str(key)][0]) == tuple(int(v) for v in shape), key


def test_default_spec_unchanged():
    # the dilated model's shapes (model.py:103,112-122), and dense=False is the default, bit for bit
    spec = W.vp3d_spec(filter_widths=[3, 3, 3, 3, 3])
    assert spec == W.vp3d_spec(filter_widths=[3, 3, 3, 3, 3], dense=False)
    for i in range(4):
        assert spec[f"layers_conv.{2 * i}.weight"][0] == (1024, 1024, 3)
        assert spec[f"layers_conv.{2 * i + 1}.weight"][0] == (1024, 1024, 1)
    assert spec["expand_conv.weight"][0] == (1024, 34, 3) and spec["shrink.weight"][0] == (51, 1024, 1)
    a = W.make_vp3d_state_dict(seed=0, filter_widths=[3, 5, 3])
    b = W.make_vp3d_state_dict(seed=0, filter_widths=[3, 5, 3], dense=False)
    d = W.make_vp3d_state_dict(seed=0, filter_widths=[3, 5, 3], dense=True)
    assert list(a) == list(b) == list(d)
    for k in a:
        assert torch.equal(a[k], b[k])
        if k.startswith("layers_conv.") and int(k.split(".")[1]) % 2 == 0:
            assert d[k].shape != a[k].shape
        else:   # only the wide convs differ
            assert torch.equal(a[k], d[k]), k


def test_dense_handle_and_weight_shape_check():
    """The handle (no device needed before finalize): receptive field, pads and shifts are the dilated model's; a
    checkpoint of the other kind is refused with a size mismatch that names the key, before any upload."""
    from skiing_analysis_pytorch_amd import vp3d

    for fw, causal in (([3, 3, 3], False), ([3, 3, 3, 3, 3], True), ([3, 5, 3], False)):
        md = vp3d.TemporalModel(17, 2, 17, fw, causal=causal, dense=True)
        m = vp3d.TemporalModel(17, 2, 17, fw, causal=causal)
        assert md.dense and not m.dense
        assert md.receptive_field() == m.receptive_field() == R.receptive_field(fw)
        assert (md.pad, md.causal_shift) == (m.pad, m.causal_shift) == R.pads(fw, causal)
        assert md.total_causal_shift() == m.total_causal_shift()
    fw = [3, 3, 3]
    with pytest.raises(RuntimeError, match=r"size mismatch for layers_conv\.0\.weight"):
        vp3d.TemporalModel(17, 2, 17, fw, dense=True).load_state_dict(W.make_vp3d_state_dict(seed=0, filter_widths=fw))
    with pytest.raises(RuntimeError, match=r"size mismatch for layers_conv\.0\.weight"):
        vp3d.TemporalModel(17, 2, 17, fw).load_state_dict(W.make_vp3d_state_dict(seed=0, filter_widths=fw, dense=True))


# ---- the window kernel's ISA -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def isa():
    from skiing_analysis_pytorch_amd import build as b

    if shutil.which(b.HIPCC) is None and not Path(b.HIPCC).exists():
        pytest.skip("hipcc not available")
    src = "vp3d_dense.hip"
    flags = [f for f in b.CXXFLAGS if f != "-fPIC"] + b.EXTRA_FLAGS.get(src, [])
    r = subprocess.run([b.HIPCC, *flags, "-S", "--offload-device-only", str(b.CSRC / src), "-o", "-"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout


def _body(asm, name):
    out, inside = [], False
    for ln in asm.splitlines():
        if ln.startswith(name + ":"):
            inside = True
            continue
        if inside:
            if "s_endpgm" in ln:
                return out
            ins = ln.strip()
            if ins and not ins.startswith((";", ".")):
                out.append(ins)
    raise AssertionError(f"{name} not in the ISA")


def _meta(asm, name):
    meta = asm[asm.index("amdhsa.kernels"):]
    for block in meta.split("\n  - "):
        if re.search(rf"\.name:\s+{re.escape(name)}\s*$", block, flags=re.M):
            return {k: int(v) for k, v in re.findall(r"\.([a-z_]+):\s+(\d+)\s*$", block, flags=re.M)}
    raise AssertionError(f"no metadata for {name}")


@pytest.mark.parametrize("ta", [1, 2])
@pytest.mark.parametrize("rt", range(1, 9))
def test_window_kernel_isa(isa, ta, rt):
    """Every (TA, RT) instance the launcher can pick: only v_mfma_f32_16x16x32_bf16, 3 TA RT of them per tap (the loop
    body may be duplicated by the compiler), no scratch, no VGPR spill, and registers for the two waves per SIMD of a
    512-thread workgroup."""
    name = f"_ZN5skimi15vp3d_win_kernelILi{ta}ELi{rt}EEEvNS_7Vp3dWinE"
    body = _body(isa, name)
    mfma = [ins.split()[0] for ins in body if ins.startswith("v_mfma")]
    assert set(mfma) == {"v_mfma_f32_16x16x32_bf16"}, sorted(set(mfma))
    assert mfma and len(mfma) % (3 * ta * rt) == 0, len(mfma)
    assert not any(ins.startswith("scratch_") for ins in body)
    m = _meta(isa, name)
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0
    assert m["vgpr_count"] <= 256, m["vgpr_count"]
