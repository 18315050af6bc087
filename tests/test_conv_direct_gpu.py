"""The direct 3x3 -> 32 convolution of the DPT heads (csrc/conv_direct.hip) as the heads launch it, against float64.

conv_direct_n32_kernel is output_conv2[0] of both heads at full resolution.  run_dpt hands it interleaved pixel records
[pixel][hi C | lo C] (in_lo = in_hi + C, px_stride = 2 C); skimi_conv3x3_n32_strided makes that launch reachable, and
every case here runs both on two separate planes and on such records.  Every case
  * uses operands whose contraction is exact in fp32 (conv_direct_restated.py: small integers for the pure index path,
    wide integers in A or in W so that the lo planes and the a_lo.w_hi / a_hi.w_lo terms carry value; the exactness
    preconditions are asserted in test_conv_direct_cpu.py), so the result must EQUAL the float64 reference element by
    element: one wrong border pixel or one column swapped inside a tile fails, which a norm over the map would hide;
  * hands the planes over as views into NaN-filled buffers (64 NaN pixels in front of the first frame and behind the
    last): a halo pixel fetched from memory where the zero page belongs turns the output NaN or, at a frame seam,
    into the neighbour frame's value;
  * writes into a NaN-guarded output whose guards must stay NaN.

(F, H, W, C) of SHAPES, each the smallest that still shows its hazard:
  (1, 1, 1, 32)     a one-pixel image: all eight neighbours come from the zero page; one slice, no buffer flip
  (2, 16, 16, 32)   exactly one interior tile per frame: the interior store path
  (3, 16, 16, 64)   frame seams at full tiles: halo rows y = -1 and y = 16 of the middle frame are zero, not a neighbour
  (3, 17, 15, 64)   ragged right and bottom; H one over a tile: the second tile row has one valid row
  (1, 33, 18, 96)   odd slice count (the buffer parity at exit); W equals the 18-pixel window pitch
  (2, 5, 40, 128)   H smaller than a tile, several tiles across
  (1, 48, 32, 256)  interior tiles only, 8 slices, the largest K (the exactness bound)

Random data is compared per element with the bf16x3 error model of test_gemm_epilogue_gpu.run_case; the worst
error / bound ratios are recorded in profiles/conv_direct_tests.md."""
import functools
import math

import pytest
import torch

import conv_direct_restated as R
from skiing_analysis_pytorch_amd import ops
from skiing_analysis_pytorch_amd._lib import ACT_NONE, ACT_RELU, PREC_BF16X3, SkimiError
from test_gemm_epilogue_gpu import U, chain

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64   # NaN pixels in front of the first frame and behind the last one
LAYOUTS = ("planes", "interleaved")
MODES = ((True, False), (True, True), (False, False))   # (bias, relu)


def _sid(shape):
    return "x".join(map(str, shape))


def _mode(shape, family, layout):
    """(bias, relu) of an exact case: each shape meets all three modes in each layout"""
    return MODES[(R.SHAPES.index(shape) + R.FAMILIES.index(family) + LAYOUTS.index(layout)) % 3]


for _l in LAYOUTS:   # relu = 0, relu = 1 and bias = None each occur with each layout
    assert {_mode(s, f, _l) for s in R.SHAPES for f in R.FAMILIES} == set(MODES)


@functools.lru_cache(maxsize=None)
def _exact_case(family, shape, bias, relu):
    """(x, w, bias, reference) float64 on the CPU: built once, shared by the layouts, never written"""
    x, w, b = R.exact_operands(family, shape, seed=100 + R.SHAPES.index(shape), bias=bias)
    return x, w, b, R.reference(x, w, b, relu)


def _launch(shape, hi, lo, layout, packed, bias, relu):
    """one launch on planes hi / lo [F, H, W, C] (bf16, CPU) laid out as `layout` inside NaN guards -> (the result on
    the CPU, the whole guarded output buffer)"""
    F_, H, W_, C = shape
    if layout == "planes":
        (hv, _), (lv, _) = R.guarded(hi, GUARD, DEV), R.guarded(lo, GUARD, DEV)
        planes, px_stride = (hv, lv), None
    else:
        rv, _ = R.guarded(R.interleave(hi, lo), GUARD, DEV)
        planes, px_stride = (rv, rv.view(-1)[C:]), 2 * C
    ov, obuf = R.guarded(torch.full((F_, H, W_, 32), float("nan")), GUARD, DEV)
    got = ops.conv3x3_n32(shape, None, bias, relu, planes=planes, px_stride=px_stride, packed=packed, out=ov)
    torch.cuda.synchronize()
    assert got is ov
    return ov.cpu(), obuf.cpu()


def _guards_intact(obuf, what):
    n = GUARD * 32
    assert torch.isnan(obuf[:n]).all(), f"{what}: elements in front of the output were written"
    assert torch.isnan(obuf[-n:]).all(), f"{what}: elements behind the output were written"


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("shape", R.SHAPES, ids=_sid)
def test_exact(shape, family, layout):
    bias, relu = _mode(shape, family, layout)
    x, w, b, ref = _exact_case(family, shape, bias, relu)
    hi, lo = R.split_hi_lo(x)
    packed = ops.conv3x3_n32_pack(w.float().to(DEV))
    got, obuf = _launch(shape, hi, lo, layout, packed, b.float().to(DEV) if bias else None, relu)
    what = f"{_sid(shape)} {family} {layout} bias={bias} relu={relu}"
    count, first = R.first_wrong(got.double(), ref)
    assert count == 0, f"{what}: {count} of {ref.numel()} elements differ from the float64 reference; first at " \
                       f"(f, y, x, co) = {first}: got {got[first].item()!r}, want {ref[first].item()!r}"
    assert torch.equal(got.double(), ref)
    _guards_intact(obuf, what)


@pytest.mark.parametrize("shape", [(3, 17, 15, 64), (1, 33, 18, 96)], ids=_sid)
def test_interleaved_matches_planes_bitwise(shape):
    """the records as run_dpt makes them: the coarse map upsampled (+ UV tables) straight into [pixel][hi C | lo C].
    The conv on those records and on the two planes copied out of them is the same kernel summing in the same order."""
    F_, H, W_, C = shape
    g = R.gen(40 + C)
    coarse = torch.randn(F_, (H + 1) // 2, (W_ + 1) // 2, C, generator=g).to(DEV)
    tabx = (0.1 * torch.randn(W_, C // 2, generator=g)).to(DEV)
    taby = (0.1 * torch.randn(H, C // 2, generator=g)).to(DEV)
    w = torch.randn(32, C, 3, 3, generator=g) / math.sqrt(9 * C)
    b = torch.randn(32, generator=g).to(DEV)
    packed = ops.conv3x3_n32_pack(w.to(DEV))
    rv, rbuf = R.guarded(torch.zeros(F_, H, W_, 2 * C, dtype=torch.bfloat16), GUARD, DEV)
    ops.resize_bilinear_planes(coarse, H, W_, rv, tabx=tabx, taby=taby, records=False)
    torch.cuda.synchronize()
    assert not torch.isnan(rv).any() and torch.isnan(rbuf[:GUARD * 2 * C]).all() and torch.isnan(rbuf[-GUARD * 2 * C:]).all()
    assert (rv[..., C:].float() != 0).float().mean() > 0.5, "the lo halves must carry value"
    ov, obuf = R.guarded(torch.full((F_, H, W_, 32), float("nan")), GUARD, DEV)
    ops.conv3x3_n32(shape, None, b, True, planes=(rv, rv.view(-1)[C:]), px_stride=2 * C, packed=packed, out=ov)
    sep = ops.conv3x3_n32(shape, None, b, True, planes=(rv[..., :C].contiguous(), rv[..., C:].contiguous()), packed=packed)
    torch.cuda.synchronize()
    assert torch.isfinite(ov).all() and (ov > 0).any()
    assert torch.equal(ov.view(torch.int32), sep.view(torch.int32)), \
        f"{int((ov.view(torch.int32) != sep.view(torch.int32)).sum())} elements differ between the two layouts"
    _guards_intact(obuf.cpu(), "interleaved")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", [(3, 17, 15, 64), (1, 48, 32, 256)], ids=_sid)
def test_random_against_error_model(shape, layout):
    """acc_err of test_gemm_epilogue_gpu.run_case for bf16x3: the dropped lo * lo term and the lo halves' own rounding
    (2^-15) and K = 9 C fp32 sums, on sum |a| |w|; the bias add and the ReLU through chain().  Per element.
    Worst error / bound on the MI355X: 0.0100 at C = 64, 0.0021 at C = 256, the same in both layouts."""
    F_, H, W_, C = shape
    relu = C == 64
    g = R.gen(60 + C)
    x = torch.randn(shape, generator=g)
    w = torch.randn(32, C, 3, 3, generator=g) / math.sqrt(9 * C)
    b = torch.randn(32, generator=g)
    acc = R.reference(x.double(), w.double()).view(-1, 32)
    mag = R.reference(x.double().abs(), w.double().abs()).view(-1, 32)
    val, err = chain(acc, (2.0 ** -15 + 9 * C * U) * mag, bias=b, act=ACT_RELU if relu else ACT_NONE)
    hi, lo = R.split_hi_lo(x)
    got, obuf = _launch(shape, hi, lo, layout, ops.conv3x3_n32_pack(w.to(DEV)), b.to(DEV), relu)
    d = (got.double().view(-1, 32) - val).abs()
    ratio = float((d / err).nan_to_num(nan=float("inf")).max())
    print(f"conv_direct random {_sid(shape)} {layout}: worst error / bound = {ratio:.4f} (max abs error {float(d.max()):.3e})")
    bad = ~(d <= err)
    assert not bad.any(), f"{int(bad.sum())} of {bad.numel()} elements outside the bound, worst error / bound {ratio:.3f}"
    _guards_intact(obuf, f"random {_sid(shape)} {layout}")


def test_agrees_with_generic_kernel_on_integers():
    """the kernel the heads fall back to under SKIMI_CONV_DIRECT=0: the generic implicit-gather GEMM gives the same bits"""
    shape = (2, 5, 40, 128)
    F_, H, W_, C = shape
    x, w, b, ref = _exact_case("ints_small", shape, True, False)
    hi, lo = R.split_hi_lo(x)
    direct, _ = _launch(shape, hi, lo, "planes", ops.conv3x3_n32_pack(w.float().to(DEV)), b.float().to(DEV), False)
    wp = w.float().permute(0, 2, 3, 1).reshape(32, 9 * C).contiguous().to(DEV)   # [Cout, ky, kx, Cin]
    conv = dict(N=F_, H=H, W=W_, C=C, KH=3, KW=3, stride=1, pad=1, dil=1, OH=H, OW=W_)
    out = ops.gemm(x.float().reshape(-1, C).to(DEV), wp, prec=PREC_BF16X3, bias=b.float().to(DEV), conv=conv)
    path = ops.gemm_last_path()
    torch.cuda.synchronize()
    assert path.family == "generic" and path.splitk == 1, path
    assert torch.equal(out.cpu().view(torch.int32), direct.reshape(-1, 32).view(torch.int32))
    assert torch.equal(direct.double(), ref)


@pytest.mark.parametrize("C", [32, 96, 256])
def test_pack_bit_exact(C):
    """conv_direct_pack_kernel against the documented layout; 32 * C * 9 = 73728 elements at C = 256 against the
    launch's 16384 threads: the grid-stride loop runs 4.5 times.  Weights over 13 binades, exact zeros, and values
    that are bf16 numbers already (lo == 0)."""
    g = R.gen(80 + C)
    w = torch.randn(32, C, 3, 3, generator=g) * 2.0 ** torch.randint(-6, 7, (32, C, 3, 3), generator=g).float()
    w[torch.rand(w.shape, generator=g) < 0.05] = 0.0
    exact = torch.rand(w.shape, generator=g) < 0.1
    w[exact] = w[exact].to(torch.bfloat16).float()
    want = R.pack_restated(w)
    assert (want[:, 1].float() != 0).float().mean() > 0.5 and (want[:, 1].float() == 0).float().mean() > 0.1
    got = ops.conv3x3_n32_pack(w.to(DEV))
    torch.cuda.synchronize()
    assert got.shape == want.shape and got.dtype == torch.bfloat16
    diff = got.cpu().view(torch.int16) != want.view(torch.int16)
    assert not diff.any(), f"{int(diff.sum())} packed elements differ; first at [slice, plane, tap, cout, cin % 32] = " \
                           f"{tuple(int(i) for i in diff.nonzero()[0])}"


def test_bad_arguments_are_rejected():
    """every refusal is SKIMI_ERR_ARG with a message, and nothing is launched: the NaN-filled output stays NaN"""
    shape = (2, 16, 16, 32)
    F_, H, W_, C = shape
    hi, lo = R.split_hi_lo(torch.randn(F_, H, W_, 2 * C, generator=R.gen(3)))   # room for every variant below
    (hv, _), (lv, _) = R.guarded(hi, GUARD, DEV), R.guarded(lo, GUARD, DEV)
    packed = torch.zeros(2 * 32 * 64 * 9, dtype=torch.bfloat16, device=DEV)
    out = torch.full((F_, H, W_, 32), float("nan"), device=DEV)
    ops.conv3x3_n32(shape, None, planes=(hv, lv), px_stride=2 * C, packed=packed, out=out)   # the arguments are good ...
    torch.cuda.synchronize()
    assert not torch.isnan(out).any()
    out.fill_(float("nan"))
    off1 = hv.view(-1)[1:]
    cases = {
        "C = 48": (dict(x=(F_, H, W_, 48), planes=(hv, lv), px_stride=None), "bad shape"),
        "C = 0": (dict(x=(F_, H, W_, 0), planes=(hv, lv), px_stride=None), "bad shape"),
        "null hi plane": (dict(x=shape, planes=(None, lv), px_stride=None), "null buffer"),
        "null lo plane": (dict(x=shape, planes=(hv, None), px_stride=2 * C), "null buffer"),
        "hi plane off by one element": (dict(x=shape, planes=(off1, lv), px_stride=None), "16-B alignment"),
        "lo plane off by one element": (dict(x=shape, planes=(hv, off1), px_stride=2 * C), "16-B alignment"),
        "px_stride < C": (dict(x=shape, planes=(hv, lv), px_stride=C - 8), "px_stride < C"),
        "px_stride = C + 4": (dict(x=shape, planes=(hv, lv), px_stride=C + 4), "px_stride % 8"),
        "px_stride = 0": (dict(x=shape, planes=(hv, lv), px_stride=0), "px_stride must be positive"),
    }
    for name, (kw, msg) in cases.items():   # ... until one of them is not
        with pytest.raises(SkimiError, match=msg) as e:
            ops.conv3x3_n32(kw["x"], None, planes=kw["planes"], px_stride=kw["px_stride"], packed=packed, out=out)
        assert "failed" in str(e.value), name
        torch.cuda.synchronize()
        assert torch.isnan(out).all(), f"{name}: the refused call wrote to the output"
    with pytest.raises(SkimiError, match="32"):   # the pack refuses what the conv would refuse
        ops.conv3x3_n32_pack(torch.zeros(32, 48, 3, 3, device=DEV))
