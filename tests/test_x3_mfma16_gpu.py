"""GPU: the bf16x3 DPT-head kernels (gemm_x3dma.hip) on both MFMA shapes (SKIMI_X3_MFMA = 16 | 32): the fast
epilogue's variants on each shape against float64 (run_case of test_gemm_epilogue_gpu), and exact-integer operands --
every A form (plain rows, A records, tap-major and slice-major conv gather), wide and narrow tiles, ragged M / N, one
to many K-tiles -- bit-identical between the two shapes and equal to the exact float64 result."""
import pytest
import torch
import torch.nn.functional as F

from skiing_analysis_pytorch_amd import ops
from skiing_analysis_pytorch_amd._lib import ACT_RELU, PREC_BF16X3
from test_gemm_epilogue_gpu import X3_FAST, X3_SHAPES, X3_VARIANTS, _x3_features, run_case

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = ("16", "32")


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("variant,kind,a_form", X3_FAST)
def test_x3_fast_epilogue_each_shape(variant, kind, a_form, shape, monkeypatch):
    res, o, rc = X3_VARIANTS[variant]
    c = dict(X3_SHAPES[kind], **_x3_features(res, o, rc, variant))
    if a_form == "conv":
        c.pop("M")
        c["conv"] = dict(N=2, H=18, W=17, C=32, KH=3, KW=3, stride=1, pad=1)
    else:
        c["K"] = 160
    run_case(monkeypatch, **c, w_split=True, a_records=a_form == "records",
             env={"SKIMI_X3_MIN_TILES": 1, "SKIMI_X3_MFMA": shape}, seed=variant,
             expect=dict(family="x3dma_" + kind, splitk=1, mfma=int(shape)))


def _ints(shape, lim, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-lim, lim + 1, shape, generator=g).double()


def _records(x):
    ar = ops.records_buffer(*x.shape)
    nrec = x.shape[0] * ((x.shape[1] + 31) // 32) * 64
    ar[:nrec] = ops.split_records(x).reshape(-1)
    ar[nrec:] = 0
    return ar


# (A form, M or conv geometry (images, H, W, C), N, K or None, seed); K-tile counts 1, 2, 3, 4 and many
CASES = {
    "rows_k1": ("rows", 612, 352, 32), "rows_k2": ("rows", 612, 128, 64), "rows_k3": ("rows", 700, 300, 96),
    "rows_k4": ("rows", 530, 100, 128), "rows_long": ("rows", 1100, 520, 2048), "rows_long_n": ("rows", 1100, 128, 2048),
    "records_long": ("records", 900, 384, 1024), "records_long_n": ("records", 900, 120, 1024),
    "conv_tap": ("conv_tap", (2, 19, 23, 64), 256, None), "conv_tap_n": ("conv_tap", (2, 19, 23, 64), 128, None),
    "conv_slice": ("conv_slice", (2, 37, 29, 256), 272, None), "conv_slice_n": ("conv_slice", (3, 40, 31, 256), 128, None),
}


@pytest.mark.parametrize("case", list(CASES))
def test_x3_shapes_bit_identical(case, monkeypatch):
    form, geo, N, K = CASES[case]
    monkeypatch.setenv("SKIMI_X3_MIN_TILES", "1")
    seed = list(CASES).index(case)
    conv = None
    if form.startswith("conv"):
        n, H, W, C = geo
        conv = dict(N=n, H=H, W=W, C=C, KH=3, KW=3, stride=1, pad=1, dil=1, OH=H, OW=W)
        M, K, a_shape = n * H * W, 9 * C, (n * H * W, C)
    else:
        M, a_shape = geo, (geo, K)
    # integers (exact in bf16: lo halves 0) and weights scaled so that every fp32 partial sum is exact
    a64 = _ints(a_shape, 3, 100 + seed)
    w64 = _ints((N, K), 7, 200 + seed) * 2.0 ** -6
    b64 = _ints((N,), 40, 300 + seed) * 2.0 ** -4
    r64 = _ints((M, N), 40, 400 + seed) * 2.0 ** -4
    if conv is not None:
        x = a64.view(n, H, W, C).permute(0, 3, 1, 2)
        wk = w64.view(N, 3, 3, C).permute(0, 3, 1, 2)
        acc = F.conv2d(x, wk, padding=1).permute(0, 2, 3, 1).reshape(M, N)
    else:
        acc = a64 @ w64.T
    want = (acc + b64).clamp_min(0) + r64
    w_dev = w64
    if form == "conv_slice":   # weights [Cout][Cin / 32][ky][kx][32]
        w_dev = w64.view(N, 3, 3, C // 32, 32).permute(0, 3, 1, 2, 4).reshape(N, K)
        conv["slice_major"] = True
    a_t, w_t = a64.float().to(DEV), w_dev.float().to(DEV)
    b_t, r_t = b64.float().to(DEV), r64.float().to(DEV)
    kw = dict(w_split=ops.split_records(w_t))
    if form == "records":
        kw.update(a_records=_records(a_t), M=M, lda=K)
    else:
        kw["x3_scratch"] = torch.empty(ops.x3_scratch_numel(*a_shape), dtype=torch.float32, device=DEV)
    if conv is not None:
        kw["conv"] = conv
    got = {}
    for shape in SHAPES:
        monkeypatch.setenv("SKIMI_X3_MFMA", shape)
        o = torch.full((M, N), float("nan"), device=DEV)
        ops.gemm(None if form == "records" else a_t, w_t, prec=PREC_BF16X3, bias=b_t, act=ACT_RELU, resid=r_t, out=o, **kw)
        path = ops.gemm_last_path()
        assert path.family == ("x3dma_narrow" if N <= 128 else "x3dma_wide") and path.mfma == int(shape), path
        got[shape] = o
    torch.cuda.synchronize()
    assert torch.equal(got["16"], got["32"]), int((got["16"] != got["32"]).sum())
    assert torch.equal(got["16"].double().cpu(), want), float((got["16"].double().cpu() - want).abs().max())
