"""Which kernel skimi_gemm picks, pinned row by row: the planning of gemm_dispatch (csrc/gemm.hip) and of the family
launchers it hands off to (gemm256_launch, gemm_x3dma_eligible, conv_win_eligible).

TABLE holds one descriptor on each side of every threshold of that planning.  Each is launched once through ops.gemm on
small seeded operands and the only thing looked at is ops.gemm_last_path(): it must equal the value recorded in
tests/golden/gemm_dispatch.json.  Numerics are the business of test_gemm_epilogue_gpu / test_gemm_gather_gpu.

The golden is never written by the tree under test: `python tests/test_gemm_dispatch_gpu.py`, run at the commit one
compares against with that commit's library, prints the table as JSON.

SKIMI_SPLITK_ATOMIC is read once per process, so the ATOMIC rows run in a child process that has it set
(test_dispatch_table_splitk_atomic; one child for all of them).

Left out, because no descriptor reaches them: the clauses of conv_win_eligible that an earlier SKIMI_CHECK_ARG of
gemm_dispatch already rejects (16-bit lda / ldw % 8, cC % 32 and cC < 32 behind "cC % 64", records and a missing `out`
behind "out_records is an output form of the fp32-accurate mode"), and its two 2^31-element limits (4 GB operands)."""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
if __name__ == "__main__":
    sys.path.insert(0, str(ROOT))
    os.environ.setdefault("SKIMI_ENV_DYNAMIC", "1")   # as tests/conftest.py sets it

from skiing_analysis_pytorch_amd import ops  # noqa: E402
from skiing_analysis_pytorch_amd._lib import ACT_GELU, ACT_NONE, PREC_BF16, PREC_BF16X3, PREC_F16  # noqa: E402

DEV = "cuda"
GOLDEN = ROOT / "tests" / "golden" / "gemm_dispatch.json"
f32, bf16, f16 = torch.float32, torch.bfloat16, torch.float16
# switches that would move a threshold: the table is recorded with all of them unset
SWITCHES = ("SKIMI_GEMM256_MT3", "SKIMI_GEMM256_W4", "SKIMI_GEMM256_PP", "SKIMI_GEMM256_MFMA", "SKIMI_GEMM256_DEEP",
            "SKIMI_X3_MIN_TILES", "SKIMI_X3_MFMA", "SKIMI_CONV_WIN")


def _row(M=None, N=None, K=None, prec=PREC_BF16, a=f32, w=f32, out=f32, **kw):
    return dict(M=M, N=N, K=K, prec=prec, a=a, w=w, out=out, **kw)


def _g256(M=2048, N=512, K=64, a=bf16, out=bf16, **kw):
    """bf16 x bf16 plain rows: the 256-row kernels of gemm256.hip from M = 2048, N = 512, K % 64 == 0"""
    return _row(M, N, K, a=a, w=bf16, out=out, **kw)


def _x3(M, N):
    """fp32 operands with the weights also as records (W_split) and scratch for the A records"""
    return _row(M, N, 32, prec=PREC_BF16X3, w_split=True)


def _cw(n=2, H=256, W=256, C=64, KH=3, KW=3, stride=1, pad=1, dil=1, N=128, a=bf16, out=bf16, **kw):
    """3 x 3 / stride 1 / pad 1 to 128 channels on bf16: conv_win.hip where 512 whole 16 x 16 tiles dominate"""
    return _row(N=N, a=a, w=a, out=out, conv=dict(N=n, H=H, W=W, C=C, KH=KH, KW=KW, stride=stride, pad=pad, dil=dil), **kw)


TABLE = {
    # ---- generic kernel: tile -------------------------------------------------------------------------------------
    "tile_127_of_128x128": _row(127 * 128, 128, 64),          # cdiv(M, 128) * cdiv(N, 128) = 127: 64-row tile
    "tile_128_of_128x128": _row(128 * 128, 128, 64),
    "tile_128x64_n64": _row(128 * 128, 64, 64),               # BM = 128 and N <= 64
    "tile_128x64_n68": _row(128 * 128, 68, 64),
    # ---- split-K: tiles < 192, nkt >= 8, a scratch of at least one plane ------------------------------------------
    "splitk_191_tiles": _row(64 * 191, 64, 512, planes=2),
    "splitk_192_tiles": _row(64 * 192, 64, 512, planes=2),
    "splitk_nkt7": _row(64, 64, 448, planes=2),
    "splitk_nkt8": _row(64, 64, 512, planes=2),
    "splitk_nkt8_x3": _row(64, 64, 256, prec=PREC_BF16X3, planes=2),   # K-tile of 32
    "splitk_no_scratch": _row(64, 64, 512),
    "splitk_scratch_under_a_plane": _row(64, 64, 512, planes=0.5),
    "splitk_4_planes": _row(64, 64, 1024, planes=4),          # min(cdiv(512, tiles), nkt / 4) = 4
    "splitk_3_planes": _row(64, 64, 1024, planes=3),          # one plane fewer than that
    "splitk_forced_ordered": _row(64, 64, 512, planes=3, force_splitk=3),
    "splitk_forced_one_plane": _row(64, 64, 512, planes=1, force_splitk=3),   # atomics
    "splitk_forced_off_gemm256": _g256(planes=2, force_splitk=2),             # a pinned count keeps the generic kernel
    # ---- gemm256: eligibility --------------------------------------------------------------------------------------
    "g256_m2047": _g256(M=2047),
    "g256_m2048": _g256(),
    "g256_n511": _g256(N=511),
    "g256_k72": _g256(K=72),
    "g256_a_fp32": _g256(a=f32),
    # the 192-row tile: cost(bm) = ceil(cdiv(M, bm) * cdiv(N, 256) / 256) * bm, taken when cost(192) < 0.8 cost(256)
    "g256_rounds_differ": _g256(M=128 * 256),                 # 256 tiles: 1 round of 256 rows against 2 of 192
    "g256_rounds_tie": _g256(M=129 * 256),                    # 258 / 344 tiles: 2 rounds either way, 384 < 0.8 * 512
    "g256_rounds_tie_f16": _row(129 * 256, 512, 64, prec=PREC_F16, a=f16, w=f16, out=f16),
    # single-stream against ping-pong loop, at the M where the 256-row tile is taken (a single round of either tile
    # always goes to the 192-row one: 192 < 0.8 * 256)
    "g256_epi0": _g256(M=128 * 256, out=f32),
    "g256_epi1": _g256(M=128 * 256, bias=True),
    "g256_epi2_k1024": _g256(M=128 * 256, K=1024, out=f32, gamma=True, resid=True),
    "g256_epi2_k1088": _g256(M=128 * 256, K=1088, out=f32, gamma=True, resid=True),
    "g256_epi3": _g256(M=128 * 256, bias=True, act=ACT_GELU),
    "g256_f16": _row(128 * 256, 512, 64, prec=PREC_F16, a=f16, w=f16, out=f16),
    "g256_f16_gelu": _row(128 * 256, 512, 64, prec=PREC_F16, a=f16, w=f16, out=f16, bias=True, act=ACT_GELU),
    # ---- bf16x3 LDS-DMA: 160 tiles of 256 rows, N >= 96, narrow loop to N = 128 -----------------------------------
    "x3_159_tiles": _x3(256 * 159, 256),
    "x3_160_tiles": _x3(256 * 160, 256),
    "x3_n128": _x3(256 * 160, 128),
    "x3_n129": _x3(256 * 160, 129),
    "x3_n95": _x3(256 * 160, 95),
    "x3_n96": _x3(256 * 160, 96),
    "x3_no_w_split": _row(256 * 160, 256, 32, prec=PREC_BF16X3),
    # ---- conv_win: one eligible geometry, then one row per reason of conv_win_eligible ----------------------------
    "cw_eligible": _cw(),
    "cw_f16": _cw(a=f16, prec=PREC_F16, out=f16),
    "cw_a_fp32": _row(N=128, a=f32, w=bf16, out=bf16, conv=dict(N=2, H=256, W=256, C=64, KH=3, KW=3, stride=1, pad=1, dil=1)),
    "cw_kw2": _cw(KW=2),
    "cw_stride2": _cw(stride=2),
    "cw_pad0": _cw(pad=0),
    "cw_dil2_pad2": _cw(dil=2, pad=2),
    "cw_n96": _cw(N=96),
    "cw_n256": _cw(N=256),
    "cw_pixel_shuffle": _cw(pixel_shuffle=2),
    "cw_force_splitk": _cw(planes=1, force_splitk=1),
    "cw_a_misaligned": _cw(a_off=4),                          # 8 bytes
    "cw_ldo_130": _cw(ldo_pad=2),
    "cw_out_misaligned": _cw(out_off=2),                      # 4 bytes, bf16 rows want 8
    "cw_out2_misaligned": _cw(out2_off=2),                    # 8 bytes, the fp32 copy wants 16
    "cw_bias_misaligned": _cw(bias=True, bias_off=1),
    "cw_gamma_misaligned": _cw(gamma=True, gamma_off=1),
    "cw_resid_ldr_130": _cw(resid=True, ldr_pad=2),
    "cw_511_tiles": _cw(n=7, H=16 * 73, W=16),
    "cw_512_tiles": _cw(n=8, H=16 * 64, W=16),
    "cw_ragged_tiles": _cw(n=128, H=17, W=17),                # 512 tiles of which 289 / 1024 of the pixels exist
}

# SKIMI_SPLITK_ATOMIC=1 (child process)
ATOMIC = {
    "atomic_forced": _row(64, 64, 512, planes=3, force_splitk=3),
    "atomic_one_plane_4_splits": _row(64, 64, 1024, planes=1),   # the plane count no longer bounds the split count
    "atomic_no_scratch": _row(64, 64, 1024),
}


def launch(r):
    """one ops.gemm launch of table row `r`; returns the raw skimi_gemm_last_path value"""
    g = torch.Generator(device=DEV).manual_seed(0)

    def rand(rows, cols, dt, off=0, ld_pad=0):   # [rows, cols] view, row stride cols + ld_pad, `off` elements into its buffer
        buf = torch.randn(rows * (cols + ld_pad) + off, generator=g, device=DEV).to(dt)
        return buf[off:].view(rows, cols + ld_pad)[:, :cols]

    M, N, K, cv = r["M"], r["N"], r["K"], r.get("conv")
    kw = {}
    if cv is not None:
        cv = dict(cv)
        cv["OH"] = (cv["H"] + 2 * cv["pad"] - cv["dil"] * (cv["KH"] - 1) - 1) // cv["stride"] + 1
        cv["OW"] = (cv["W"] + 2 * cv["pad"] - cv["dil"] * (cv["KW"] - 1) - 1) // cv["stride"] + 1
        M, K = cv["N"] * cv["OH"] * cv["OW"], cv["KH"] * cv["KW"] * cv["C"]
        a = rand(cv["N"] * cv["H"] * cv["W"], cv["C"], r["a"], off=r.get("a_off", 0))
        kw["conv"] = cv
    else:
        a = rand(M, K, r["a"])
    w = rand(N, K, r["w"])
    out_rows, out_cols = M, N
    if r.get("pixel_shuffle"):
        s = r["pixel_shuffle"]
        kw["pixel_shuffle"] = (s, N // (s * s), cv["N"], cv["H"], cv["W"])
        out_rows, out_cols = M * s * s, N // (s * s)
    out = rand(out_rows, out_cols, r["out"], off=r.get("out_off", 0), ld_pad=r.get("ldo_pad", 0))
    if "out2_off" in r:
        kw["out2"] = rand(M, N, f32 if r["out"] != f32 else bf16, off=r["out2_off"])
    if r.get("bias"):
        kw["bias"] = rand(1, N, f32, off=r.get("bias_off", 0))[0]
    if r.get("gamma"):
        kw["gamma"] = rand(1, N, f32, off=r.get("gamma_off", 0))[0]
    if r.get("resid"):
        kw["resid"] = rand(M, N, f32, ld_pad=r.get("ldr_pad", 0))
    if r.get("planes"):
        kw["splitk_scratch"] = torch.zeros(int(r["planes"] * M * N), device=DEV)
    if r.get("w_split"):
        kw["w_split"] = ops.split_records(w)
        kw["x3_scratch"] = torch.empty(ops.x3_scratch_numel(M, K), dtype=f32, device=DEV)
    ops.gemm(a, w, prec=r["prec"], act=r.get("act", ACT_NONE), out=out, force_splitk=r.get("force_splitk", 0), **kw)
    raw = ops.gemm_last_path().raw
    torch.cuda.synchronize()
    return raw


def run_rows(rows):
    return {name: launch(r) for name, r in rows.items()}


def run_atomic_child():
    """the ATOMIC rows in a fresh process with SKIMI_SPLITK_ATOMIC=1"""
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env["SKIMI_SPLITK_ATOMIC"] = "1"
    p = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--atomic-rows"], env=env, capture_output=True,
                       text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    return json.loads(p.stdout.strip().splitlines()[-1])


gpu = pytest.mark.gpu


def _golden():
    return json.loads(GOLDEN.read_text())


def _check(name, got, want):
    assert got == want, f"{name}: dispatched to {got:#x}, recorded {want:#x} (family | tile << 4 | mfma << 8 | epi << 12 | splitk << 16)"


def test_table_and_golden_have_the_same_rows():
    assert sorted(_golden()) == sorted([*TABLE, *ATOMIC])


@gpu
@pytest.mark.parametrize("name", list(TABLE))
def test_dispatch_table(monkeypatch, name):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    _check(name, launch(TABLE[name]), _golden()[name])


@gpu
def test_dispatch_table_splitk_atomic():
    got, want = run_atomic_child(), _golden()
    assert sorted(got) == sorted(ATOMIC)
    for name in ATOMIC:
        _check(name, got[name], want[name])


if __name__ == "__main__":
    for k in SWITCHES:
        os.environ.pop(k, None)
    if "--atomic-rows" in sys.argv:
        assert os.environ.get("SKIMI_SPLITK_ATOMIC") == "1"
        print(json.dumps(run_rows(ATOMIC)))
    else:
        os.environ.pop("SKIMI_SPLITK_ATOMIC", None)
        table = run_rows(TABLE)
        table.update(run_atomic_child())
        print(json.dumps(table, indent=1))
