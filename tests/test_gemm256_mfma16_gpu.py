"""GPU: the single-stream and ping-pong 256x256 loops on both MFMA shapes (SKIMI_GEMM256_MFMA = 16 | 32), every
compile-time epilogue and the generic one, fp16 and bf16 operands, ragged M / N and K = 64 .. 1024: each against an
fp64 reference, the two shapes against each other (they differ only in fp32 accumulation order), exact-integer
operands bit-identical in both, and repeated launches in one process bit-identical."""
import math

import pytest
import torch
import torch.nn.functional as F

from skiing_analysis_pytorch_amd import ops
from skiing_analysis_pytorch_amd._lib import ACT_GELU, PREC_BF16, PREC_F16

pytestmark = pytest.mark.gpu
DEV = "cuda"
LOOPS = {"single_stream": {"SKIMI_GEMM256_MT3": "0", "SKIMI_GEMM256_W4": "1"},
         "ping_pong": {"SKIMI_GEMM256_MT3": "0", "SKIMI_GEMM256_W4": "0"}}
FMT = {"f16": (torch.float16, PREC_F16), "bf16": (torch.bfloat16, PREC_BF16)}


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


def _epilogues(a, w, b, g, r, prec, dt):
    """(name, output, fp64 reference, relative tolerance) of each epilogue kind"""
    ref = a.double() @ w.double().T
    b64, g64, r64 = b.double(), g.double(), r.double()
    out = []
    o = ops.gemm(a, w, prec=prec, bias=b, out_dtype=torch.bfloat16)                           # EPI 1 (qkv)
    out.append(("bias_bf16", o, ref + b64, 1e-2))
    o = ops.gemm(a, w, prec=prec, bias=b, act=ACT_GELU, out_dtype=dt)                         # EPI 3 (fc1)
    out.append(("bias_gelu", o, F.gelu(ref + b64), 1e-3 if dt == torch.float16 else 1e-2))
    o = ops.gemm(a, w, prec=prec, bias=b, gamma=g, resid=r.clone())                           # EPI 2 (proj, fc2)
    out.append(("layerscale_resid", o, r64 + g64 * (ref + b64), 2e-5))
    o = ops.gemm(a, w, prec=prec, bias=b)                                                     # EPI 0 (generic)
    out.append(("generic_f32", o, ref + b64, 2e-5))
    return out


@pytest.mark.parametrize("fmt", list(FMT))
@pytest.mark.parametrize("loop", list(LOOPS))
@pytest.mark.parametrize("M,N,K", [(2048, 512, 64), (4300, 768, 192), (2100, 1000, 1024), (5000, 1024, 512)])
def test_mfma_shapes_agree(M, N, K, loop, fmt, monkeypatch):
    dt, prec = FMT[fmt]
    for k, v in LOOPS[loop].items():
        monkeypatch.setenv(k, v)
    a = _rand(M, K, seed=80).to(dt)
    w = _rand(N, K, seed=81, scale=1 / math.sqrt(K)).to(dt)
    b, g, r = _rand(N, seed=82), _rand(N, seed=83), _rand(M, N, seed=84)
    res = {}
    for shape in ("16", "32"):
        monkeypatch.setenv("SKIMI_GEMM256_MFMA", shape)
        res[shape] = _epilogues(a, w, b, g, r, prec, dt)
        for name, o, ref, tol in res[shape]:
            assert _rel(o.float(), ref) < tol, (shape, name)
    for (name, o16, _, tol), (_, o32, _, _) in zip(res["16"], res["32"]):
        # accumulation order only: far inside each output format's rounding
        assert _rel(o16.float(), o32.float()) < tol / 4, name
    ai = ((torch.arange(M * K, device=DEV).reshape(M, K) * 7 + 3) % 9 - 4).to(dt)
    wi = ((torch.arange(N * K, device=DEV).reshape(N, K) * 5 + 1) % 7 - 3).to(dt)
    exact = ai.double() @ wi.double().T
    for shape in ("16", "32"):
        monkeypatch.setenv("SKIMI_GEMM256_MFMA", shape)
        assert torch.equal(ops.gemm(ai, wi, prec=prec).double(), exact), shape


@pytest.mark.parametrize("fmt", list(FMT))
def test_mfma16_repeat_launches_bit_identical(fmt, monkeypatch):
    """the bench's block Linears at M = 16384 on the default shape: 12 launches of each, every one equal to the first"""
    dt, prec = FMT[fmt]
    monkeypatch.setenv("SKIMI_GEMM256_MFMA", "16")
    M = 16384
    for N, K, kind in ((3072, 1024, "qkv"), (1024, 1024, "proj"), (4096, 1024, "fc1"), (1024, 4096, "fc2")):
        a = _rand(M, K, seed=90).to(dt)
        w = _rand(N, K, seed=91, scale=1 / math.sqrt(K)).to(dt)
        b, g, r = _rand(N, seed=92), _rand(N, seed=93), _rand(M, N, seed=94)
        if kind == "qkv":
            f = lambda: ops.gemm(a, w, prec=prec, bias=b, out_dtype=torch.bfloat16)
        elif kind == "fc1":
            f = lambda: ops.gemm(a, w, prec=prec, bias=b, act=ACT_GELU, out_dtype=dt)
        else:
            f = lambda: ops.gemm(a, w, prec=prec, bias=b, gamma=g, resid=r.clone())
        first = f()
        for _ in range(11):
            assert torch.equal(f(), first), kind
