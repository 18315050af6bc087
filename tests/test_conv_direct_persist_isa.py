"""CPU: the two instantiations of conv_direct_n32_kernel (csrc/conv_direct.hip: <false> one tile per workgroup on planes in
memory, <true> the persistent tile loop that interpolates its windows) in the ISA that the build's own flags emit.

Both: one slice body of 54 v_mfma_f32_32x32x16_bf16, no VGPR spill, no scratch, registers for the 512-thread workgroup
(two waves per SIMD: at most 256 VGPRs).  The persistent loop must not wait for a tile's stores before the next tile's
MFMAs, nor for the next step's LDS-DMA before it has to: stores and LDS-DMA count in vmcnt, so the only vmcnt waits of the
kernel are the two that retire the LDS-DMA in front of a barrier (prologue, end of a step) -- the barrier between the
interpolation and the taps waits for LDS alone -- and nothing from the first store to the end of the body waits on vmcnt
or meets a barrier: from there the loop goes back to the next tile's interpolation, staging and MFMAs."""
import shutil
import subprocess
from pathlib import Path

import pytest

from test_x3_mfma16_isa import _body, _meta

NAME = "_ZN5skimi22conv_direct_n32_kernelILb{}EEEvNS_14ConvDirectArgsE"   # <UP>


@pytest.fixture(scope="module")
def isa():
    from skiing_analysis_pytorch_amd import build as b

    if shutil.which(b.HIPCC) is None and not Path(b.HIPCC).exists():
        pytest.skip("hipcc not available")
    src = "conv_direct.hip"
    flags = [f for f in b.CXXFLAGS if f != "-fPIC"] + b.EXTRA_FLAGS.get(src, [])
    r = subprocess.run([b.HIPCC, *flags, "-S", "--offload-device-only", str(b.CSRC / src), "-o", "-"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout


@pytest.mark.parametrize("up", [1, 0])
def test_registers_and_mfma_body(isa, up):
    name = NAME.format(up)
    m = _meta(isa, name)
    print(f"conv_direct_n32_kernel<{up}>:", {k: m[k] for k in ("vgpr_count", "sgpr_count", "vgpr_spill_count",
                                                                   "sgpr_spill_count", "private_segment_fixed_size")})
    assert m["vgpr_count"] <= 256 and m["vgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0
    body = _body(isa, name)
    assert not any(ins.startswith("scratch_") for ins in body)
    mfma = [ins.split()[0] for ins in body if ins.startswith("v_mfma")]
    assert set(mfma) == {"v_mfma_f32_32x32x16_bf16"} and len(mfma) == 54, (sorted(set(mfma)), len(mfma))


def test_stores_are_not_waited_for_before_the_next_tile(isa):
    body = _body(isa, NAME.format(1))
    vm = [i for i, ins in enumerate(body) if ins.startswith("s_waitcnt") and "vmcnt" in ins]
    barriers = [i for i, ins in enumerate(body) if ins.startswith("s_barrier")]
    assert len(barriers) == 3, barriers   # prologue; interpolation -> taps; end of a step
    assert [i + 1 for i in vm] == [barriers[0], barriers[2]], [body[i:i + 2] for i in vm]   # in front of the first and last
    assert "lgkmcnt(0)" in body[barriers[1] - 1] and "vmcnt" not in body[barriers[1] - 1], body[barriers[1] - 1]
    assert all("vmcnt(0)" in body[i] for i in vm)
    stores = [i for i, ins in enumerate(body) if ins.startswith("global_store_dword")]
    assert len(stores) == 16 + 1, len(stores)   # the interior tile's 16, the ragged tile's loop of one
    assert stores[0] > barriers[-1], "a barrier (and its vmcnt(0)) after the epilogue's stores"
