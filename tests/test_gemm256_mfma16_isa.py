"""CPU: the block Linears' 256x256 loops on v_mfma_f32_16x16x32 (gemm256.hip, M16 = true), checked in the ISA that the
build's own flags emit: the fp16 instantiations the bench runs -- single-stream qkv / fc2 (gemm256w4_kernel<1|2, F16, M16>)
and ping-pong fc1 / proj (gemm256pp_kernel<3|2, 1, F16, M16>) -- issue only the 16x16x32 shape, spill nothing and run at
the waves per SIMD of their 32x32x16 twins."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

KERNELS = {  # name -> (M16 mangled, 32x32 twin mangled)
    "qkv": ("_ZN5skimi16gemm256w4_kernelILi1ELb1ELb1EEEvNS_8GemmArgsE", "_ZN5skimi16gemm256w4_kernelILi1ELb1ELb0EEEvNS_8GemmArgsE"),
    "fc2": ("_ZN5skimi16gemm256w4_kernelILi2ELb1ELb1EEEvNS_8GemmArgsE", "_ZN5skimi16gemm256w4_kernelILi2ELb1ELb0EEEvNS_8GemmArgsE"),
    "fc1": ("_ZN5skimi16gemm256pp_kernelILi3ELi1ELb1ELb1EEEvNS_8GemmArgsE", "_ZN5skimi16gemm256pp_kernelILi3ELi1ELb1ELb0EEEvNS_8GemmArgsE"),
    "proj": ("_ZN5skimi16gemm256pp_kernelILi2ELi1ELb1ELb1EEEvNS_8GemmArgsE", "_ZN5skimi16gemm256pp_kernelILi2ELi1ELb1ELb0EEEvNS_8GemmArgsE"),
}


@pytest.fixture(scope="module")
def isa():
    from skiing_analysis_pytorch_amd import build as b

    if shutil.which(b.HIPCC) is None and not Path(b.HIPCC).exists():
        pytest.skip("hipcc not available")
    src = "gemm256.hip"
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


def _waves_per_simd(m):
    regs = -(-m["vgpr_count"] // 8) * 8   # unified VGPR + AGPR file of 512 per lane, granule 8
    return min(8, 512 // regs)


@pytest.mark.parametrize("kind", list(KERNELS))
def test_mfma16_loop_isa(isa, kind):
    name16, name32 = KERNELS[kind]
    body = _body(isa, name16)
    mfma = [ins.split()[0] for ins in body if ins.startswith("v_mfma")]
    assert mfma and set(mfma) == {"v_mfma_f32_16x16x32_f16"}, sorted(set(mfma))
    assert not any(ins.startswith("scratch_") for ins in body)
    m16, m32 = _meta(isa, name16), _meta(isa, name32)
    assert m16["private_segment_fixed_size"] == 0 and m16["vgpr_spill_count"] == 0 and m16["sgpr_spill_count"] == 0
    assert _waves_per_simd(m16) == _waves_per_simd(m32), (m16["vgpr_count"], m32["vgpr_count"])
    # the 32x32x16 twin (SKIMI_GEMM256_MFMA=32) is still the other shape
    assert {ins.split()[0] for ins in _body(isa, name32) if ins.startswith("v_mfma")} == {"v_mfma_f32_32x32x16_f16"}


@pytest.mark.parametrize("kind", ["qkv", "fc2"])
def test_mfma16_asm_wait_states(isa, kind):
    """the single-stream 16x16x32 loop issues its MFMAs as inline asm (hipcc pads nothing around asm): no accumulator
    register may be read, written or moved within 12 wait states of an MFMA (8-pass XDL result latency)"""
    body = _body(isa, KERNELS[kind][0])
    states = 99
    for ins in body:
        if ins.startswith("v_mfma"):
            states = 0
            continue
        if ins.startswith("v_accvgpr"):
            assert states >= 12, f"{ins} {states} states after an MFMA"
        m = re.match(r"s_nop\s+(\d+)", ins)
        states += int(m.group(1)) + 1 if m else 1
