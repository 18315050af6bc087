"""CPU: the tap-sum kernel of the DPT heads' coarse-map output_conv1 (dpt_tap_sum_kernel, vggt_kernels.hip) in the ISA
that the build's own flags emit: its 16 float4 accumulators, the register-held next window and the two interpolated
source rows stay in VGPRs (no spill, no scratch), at a budget that lets several workgroups share a CU, and the staged
window is the LDS it declares (11 x 19 coarse pixels of 128 bytes)."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

from test_x3_mfma16_isa import _body, _meta, _waves_per_simd

NAME = "_ZN5skimi18dpt_tap_sum_kernelEPKfS1_Pfiii"
LDS_BYTES = 11 * 19 * 128


@pytest.fixture(scope="module")
def isa():
    from skiing_analysis_pytorch_amd import build as b

    if shutil.which(b.HIPCC) is None and not Path(b.HIPCC).exists():
        pytest.skip("hipcc not available")
    src = "vggt_kernels.hip"
    flags = [f for f in b.CXXFLAGS if f != "-fPIC"] + b.EXTRA_FLAGS.get(src, [])
    r = subprocess.run([b.HIPCC, *flags, "-S", "--offload-device-only", str(b.CSRC / src), "-o", "-"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout


def test_tap_sum_register_budget(isa):
    m = _meta(isa, NAME)
    print("dpt_tap_sum_kernel:", {k: m[k] for k in ("vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count",
                                                    "private_segment_fixed_size", "group_segment_fixed_size")})
    assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0
    assert m["group_segment_fixed_size"] == LDS_BYTES
    # A workgroup's 4 waves sit one per SIMD.  The next window's loads are in flight in registers during a stage's sums, so
    # one workgroup already overlaps its own traffic; a second one per CU covers the two barriers of a stage.  Two per CU
    # = 2 waves per SIMD = at most 256 VGPRs, and two windows in the CU's 160 KB of LDS.
    assert m["vgpr_count"] <= 256 and _waves_per_simd(m) >= 2
    assert 160 * 1024 // LDS_BYTES >= 2


def test_tap_sum_no_scratch_and_wide_accesses(isa):
    body = _body(isa, NAME)
    assert not any(ins.startswith("scratch_") for ins in body)
    # 16-byte accesses on every path: T's windows, the LDS window, the output rows
    assert any(re.match(r"global_load_dwordx4\b", ins) for ins in body)
    assert any(re.match(r"global_store_dwordx4\b", ins) for ins in body)
    assert any(re.match(r"ds_read_b128\b|ds_load_b128\b", ins) for ins in body)
    assert any(re.match(r"ds_write_b128\b|ds_store_b128\b", ins) for ins in body)
