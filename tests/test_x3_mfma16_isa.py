"""CPU: the bf16x3 DPT-head loops on v_mfma_f32_16x16x32 (gemm_x3dma.hip, M16 = true), checked in the ISA that the
build's own flags emit: every a_mode of the 256x256 loop (gemm_x3w4_kernel<a_mode, 0, M16>) and of the 256x128 loop
(gemm_x3w4n_kernel<a_mode, M16>) issues only the 16x16x32 shape, 192 (96) MFMAs per K-tile, spills no VGPR, uses no
scratch and runs at the waves per SIMD of its 32x32x16 twin; the inline-asm MFMAs keep their accumulator wait states."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest


def _mangled(wide, a_mode, m16):
    b = int(m16)
    if wide:
        return f"_ZN5skimi16gemm_x3w4_kernelILi{a_mode}ELi0ELb{b}EEEvNS_8GemmArgsENS_5X3RecE"
    return f"_ZN5skimi17gemm_x3w4n_kernelILi{a_mode}ELb{b}EEEvNS_8GemmArgsENS_5X3RecE"


# kind -> (wide tile, MFMAs per K-tile, K-tile bodies in the code: the main loop + the peeled last two / three)
KINDS = {"wide": (True, 192, 3), "narrow": (False, 96, 4)}
CASES = [(k, a) for k in KINDS for a in (0, 1, 2)]


@pytest.fixture(scope="module")
def isa():
    from skiing_analysis_pytorch_amd import build as b

    if shutil.which(b.HIPCC) is None and not Path(b.HIPCC).exists():
        pytest.skip("hipcc not available")
    src = "gemm_x3dma.hip"
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


@pytest.mark.parametrize("kind,a_mode", CASES)
def test_x3_mfma16_isa(isa, kind, a_mode):
    wide, per_ktile, bodies = KINDS[kind]
    name16, name32 = _mangled(wide, a_mode, True), _mangled(wide, a_mode, False)
    body = _body(isa, name16)
    mfma = [ins.split()[0] for ins in body if ins.startswith("v_mfma")]
    assert set(mfma) == {"v_mfma_f32_16x16x32_bf16"}, sorted(set(mfma))
    assert len(mfma) == per_ktile * bodies, len(mfma)
    assert not any(ins.startswith("scratch_") for ins in body)
    m16, m32 = _meta(isa, name16), _meta(isa, name32)
    # (SGPR spills go to VGPR lanes, never to memory: the 32x32x16 twins carry about as many)
    assert m16["private_segment_fixed_size"] == 0 and m16["vgpr_spill_count"] == 0
    assert _waves_per_simd(m16) == _waves_per_simd(m32), (m16["vgpr_count"], m32["vgpr_count"])
    # the 32x32x16 twin (SKIMI_X3_MFMA=32) is still the other shape
    assert {ins.split()[0] for ins in _body(isa, name32) if ins.startswith("v_mfma")} == {"v_mfma_f32_32x32x16_bf16"}


@pytest.mark.parametrize("kind,a_mode", CASES)
def test_x3_mfma16_asm_wait_states(isa, kind, a_mode):
    """hipcc pads nothing around an asm statement: no accumulator register may be read, written or moved within 12
    wait states after an MFMA (8-pass XDL result latency), and an MFMA needs 2 states after a v_accvgpr_write"""
    body = _body(isa, _mangled(KINDS[kind][0], a_mode, True))
    since_mfma, since_write = 99, 99
    for ins in body:
        if ins.startswith("v_mfma"):
            assert since_write >= 2, f"{ins} {since_write} states after a v_accvgpr_write"
            since_mfma = 0
            continue
        if ins.startswith("v_accvgpr"):
            assert since_mfma >= 12, f"{ins} {since_mfma} states after an MFMA"
        m = re.match(r"s_nop\s+(\d+)", ins)
        n = int(m.group(1)) + 1 if m else 1
        since_mfma += n
        since_write = 0 if ins.startswith("v_accvgpr_write") else since_write + n
