"""CPU: the phase-folded ConvTranspose + 3x3 conv instantiation of the 256x256 bf16x3 loop (gemm_x3w4_kernel<3, 0, M16>,
gemm_x3dma.hip) in the ISA that the build's own flags emit: the same main loop as the other a_modes (192 MFMAs of the
16x16x32 shape per K-tile body), no VGPR spill, no scratch, one wave per SIMD like its 32x32x16 twin, and the
accumulator wait states of the inline-asm MFMAs kept.  The phase decode, the per-phase window and the border-class
bias select must live in scalar registers and the epilogue: a spill would show here."""
import pytest

from test_x3_mfma16_isa import _body, _meta, _waves_per_simd, isa  # noqa: F401  (isa: the module's fixture)
from test_x3_mfma16_isa import test_x3_mfma16_asm_wait_states as _wait_states
from test_x3_mfma16_isa import test_x3_mfma16_isa as _isa_case


def test_fold_isa(isa):  # noqa: F811
    _isa_case(isa, "wide", 3)


def test_fold_asm_wait_states(isa):  # noqa: F811
    _wait_states(isa, "wide", 3)


def test_fold_register_budget(isa):  # noqa: F811
    name = "_ZN5skimi16gemm_x3w4_kernelILi3ELi0ELb1EEEvNS_8GemmArgsENS_5X3RecE"
    m = _meta(isa, name)
    print("gemm_x3w4_kernel<3, 0, true>:", {k: m[k] for k in ("vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count",
                                                              "private_segment_fixed_size")})
    assert m["vgpr_count"] <= 512 and m["vgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0
    assert _waves_per_simd(m) == 1
    assert not any(ins.startswith("scratch_") for ins in _body(isa, name))
