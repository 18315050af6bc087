"""The A operand addressing of skimi_gemm (a_mode 0 / 1 / 2 of skimi_gemm_desc, include/skimi.h) on every kernel that
gathers, against a float64 reference.

The implicit im2col exists in four independent copies: ISSUE_TILE of the generic kernel (gemm.hip: three tiles x three
precisions x fp32 / 16-bit A, also under split-K, where a split starts in the middle of the tap sequence), the wide
and the narrow loop of gemm_x3dma.hip (each built for both MFMA shapes, fed by fp32 A or by A records) and conv_win.hip.
Every GPU case here
  * pins the kernel it means: ops.gemm_last_path() must name family, tile / MFMA shape and split count before any value
    is looked at;
  * uses random small integers in A and integers * 2^-k in W and the bias, so every product and every partial sum is
    exact in every precision: the result must EQUAL the float64 reference, element by element, no tolerance.  The values
    are random per position, so a tap read one pixel off cannot coincide with the right one;
  * hands A over as a view into a NaN-filled buffer: NaN pixels before the first and behind the last image, NaN in the
    columns between cC and lda, a NaN-filled x3_scratch, NaN records around the A records.  Whatever is gathered from a
    masked position without being zeroed turns the output NaN;
  * writes into a NaN sentinel buffer (row stride ldo > N): what the descriptor does not address stays NaN.
One random-data case per kernel family checks the contraction against the precision's error model (acc_err of
test_gemm_epilogue_gpu.run_case).

`gather_reference` knows nothing about tiles: it is the descriptor's documented index arithmetic, pinned on the CPU
against float64 torch.nn.functional.conv2d for every geometry of the table (test_reference_matches_conv2d)."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from skiing_analysis_pytorch_amd import ops
from skiing_analysis_pytorch_amd._lib import PREC_BF16X3, SkimiError
from test_gemm_epilogue_gpu import GEN_PRECS, H16, Sentinel, U, _env, _gen, _ints, _k_shift, chain

DEV = "cuda"
gpu = pytest.mark.gpu
GUARD = 64   # NaN pixels (rows of A) in front of the first image and behind the last one

# id: (KH, KW, stride, pad, dil), images (n, H, W) for the 64-row tile, for the 256-row tiles (257 <= M <= 700, an image
# seam in each of the two row tiles).  What each geometry is there to catch:
#   same3  image seams inside a row tile, an image smaller than a tile
#   s2     stride; the last window hangs over one edge only
#   dil2   dil on both axes, pad > 1 (a_bias of the LDS-DMA kernels)
#   valid  no padding, OH < cH
#   rect   KH != KW: ky / kx or KH / KW swapped; OW = cW + 1
#   k5     25 taps (bit 24 of the LDS-DMA kernels' tap mask)
#   vp3d_* the VideoPose3D launches (vp3d.hip: cH = 1, KH = 1, KW = k, pad 0, dilated), filter width 5 included
#   sub    1x1 stride 2: subsampling without a window
#   k6     36 taps: more than the LDS-DMA kernels' 32-bit tap mask holds
GEOMS = {
    "same3": ((3, 3, 1, 1, 1), (3, 7, 9), (3, 13, 13)),
    "s2": ((3, 3, 2, 1, 1), (5, 12, 13), (3, 26, 25)),
    "dil2": ((3, 3, 1, 2, 2), (4, 6, 7), (3, 12, 15)),
    "valid": ((3, 3, 1, 0, 1), (3, 9, 10), (3, 15, 16)),
    "rect": ((3, 2, 1, 1, 1), (3, 7, 8), (3, 13, 12)),
    "k5": ((5, 5, 1, 2, 1), (3, 7, 9), (3, 13, 14)),
    "vp3d_k3d9": ((1, 3, 1, 0, 9), (3, 1, 90), (7, 1, 90)),
    "vp3d_k5d3": ((1, 5, 1, 0, 3), (3, 1, 90), (7, 1, 90)),
    "sub": ((1, 1, 2, 0, 1), (3, 13, 15), (3, 25, 27)),
    "k6": ((6, 6, 1, 0, 1), (2, 12, 13), (3, 15, 16)),
}
X3_GEOMS = [g for g in GEOMS if g != "k6"]
C128 = {"rect"}                                                     # cC = 128 instead of 64: several K-tiles per tap
LDA_PAD = {"same3": 8, "dil2": 24, "vp3d_k3d9": 8, "sub": 16}       # lda = cC + this (a multiple of 8: fp32 and 16-bit)
# the generic kernel's larger tiles: the smallest shapes gemm_dispatch gives them (128x64: N <= 64 and cdiv(M, 128) >=
# 128; 128x128: cdiv(M, 128) * cdiv(N, 128) >= 128), M no multiple of 128
BIG = {"128x64": (60, {"same3": (3, 74, 75), "s2": (3, 148, 149), "dil2": (3, 74, 75), "rect": (3, 74, 74)}),
       "128x128": (1040, {"same3": (3, 25, 26), "s2": (3, 50, 51), "dil2": (3, 25, 26), "rect": (3, 25, 25)})}


def make_geom(name, nhw, C):
    """the descriptor's conv fields (ops.gemm's `conv` dict) of geometry `name` on n images of H x W x C"""
    (KH, KW, stride, pad, dil), (n, H, W) = GEOMS[name][0], nhw
    OH = (H + 2 * pad - dil * (KH - 1) - 1) // stride + 1
    OW = (W + 2 * pad - dil * (KW - 1) - 1) // stride + 1
    return dict(N=n, H=H, W=W, C=C, KH=KH, KW=KW, stride=stride, pad=pad, dil=dil, OH=OH, OW=OW)


def _nhw(name, size):
    return GEOMS[name][1 if size == "small" else 2] if isinstance(size, str) else size


# ---------------------------------------------------------------------------------------------------------------------
# float64 reference of the gather (skimi.h: a_mode 1 "k = (ky*KW+kx)*cC + c", a_mode 2
# "k = ((c / 32) * KH*KW + ky*KW + kx) * 32 + c % 32"; window origin o * stride - pad, taps dil apart, zero outside the
# image, an image's windows read that image only)
# ---------------------------------------------------------------------------------------------------------------------
def gather_reference(x, w, geom, slice_major=False):
    """x [cN, cH, cW, cC], w [N, K] (float64) -> gather(x) @ w.T, [cN * OH * OW, N] float64"""
    cN, cH, cW, cC = x.shape
    KH, KW, stride, pad, dil, OH, OW = (geom[k] for k in ("KH", "KW", "stride", "pad", "dil", "OH", "OW"))
    K, M = KH * KW * cC, cN * OH * OW
    assert w.shape[1] == K and x.dtype == torch.float64 and w.dtype == torch.float64
    k = torch.arange(K)
    if slice_major:
        u = k // 32
        tap, c = u % (KH * KW), (u // (KH * KW)) * 32 + k % 32
    else:
        tap, c = k // cC, k % cC
    ky, kx = tap // KW, tap % KW
    flat = x.reshape(-1)
    out = torch.empty(M, w.shape[0], dtype=torch.float64)
    for m0 in range(0, M, 4096):   # in row chunks: the im2col matrix of the largest case would be 75 MB per index array
        m = torch.arange(m0, min(M, m0 + 4096))
        img, rem = m // (OH * OW), m % (OH * OW)
        oy, ox = rem // OW, rem % OW
        iy = (oy * stride - pad)[:, None] + (ky * dil)[None, :]
        ix = (ox * stride - pad)[:, None] + (kx * dil)[None, :]
        inside = (iy >= 0) & (iy < cH) & (ix >= 0) & (ix < cW)
        src = ((img[:, None] * cH + iy.clamp(0, cH - 1)) * cW + ix.clamp(0, cW - 1)) * cC + c[None, :]
        a = torch.where(inside, flat[src], torch.zeros((), dtype=torch.float64))
        out[m0:m0 + len(m)] = a @ w.T
    return out


def _conv2d_tap_major(x, w, geom):
    """the same through torch: w [N, K] with tap-major K -> [N, C, KH, KW]"""
    wt = w.view(w.shape[0], geom["KH"], geom["KW"], geom["C"]).permute(0, 3, 1, 2)
    y = F.conv2d(x.permute(0, 3, 1, 2), wt, stride=geom["stride"], padding=geom["pad"], dilation=geom["dil"])
    assert y.shape[2:] == (geom["OH"], geom["OW"])
    return y.permute(0, 2, 3, 1).reshape(-1, w.shape[0])


@pytest.mark.parametrize("size", ["small", "x3"])
@pytest.mark.parametrize("name", list(GEOMS))
def test_reference_matches_conv2d(name, size):
    g = _gen(11 + list(GEOMS).index(name))
    for C, slice_major in ((64, False), (96, True)):
        geom = make_geom(name, _nhw(name, size), C)
        x = torch.randn(geom["N"], geom["H"], geom["W"], C, generator=g, dtype=torch.float64)
        w = torch.randn(10, geom["KH"] * geom["KW"] * C, generator=g, dtype=torch.float64)   # tap-major [N][ky][kx][C]
        want = _conv2d_tap_major(x, w, geom)
        if slice_major:   # the packing of test_gemm_conv_gather_slice_major_k: [N][C / 32][ky][kx][32]
            w4 = w.view(10, geom["KH"], geom["KW"], C).permute(0, 3, 1, 2)                  # torch's [N, C, KH, KW]
            w = w4.reshape(10, C // 32, 32, geom["KH"], geom["KW"]).permute(0, 1, 3, 4, 2).reshape(10, -1).contiguous()
        got = gather_reference(x, w, geom, slice_major)
        assert got.shape == want.shape
        assert torch.allclose(got, want, rtol=1e-12, atol=1e-12), (name, size, C, float((got - want).abs().max()))


def test_reference_seams_and_padding():
    """what conv2d cannot show on its own: a padding tap contributes exactly zero whatever lies beside the image, and an
    image's windows never read its neighbour"""
    geom = make_geom("dil2", (2, 6, 7), 32)
    g = _gen(3)
    x = torch.randn(2, 6, 7, 32, generator=g, dtype=torch.float64)
    w = torch.randn(5, 9 * 32, generator=g, dtype=torch.float64)
    both = gather_reference(x, w, geom)
    x2 = x.clone()
    x2[1] = 1e6 * torch.randn(6, 7, 32, generator=g, dtype=torch.float64)
    assert torch.equal(gather_reference(x2, w, geom)[:42], both[:42])
    assert torch.equal(gather_reference(x[:1], w, dict(geom, N=1)), both[:42])


# ---------------------------------------------------------------------------------------------------------------------
# GPU harness
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _exact_case(name, nhw, C, N, slice_major, seed):
    """(geom, x, w, bias, reference) of one exact case, float64 on the CPU; shared by every launch of the case (the
    operands are exact in bf16, fp16 and bf16x3 alike) and never modified"""
    geom = make_geom(name, nhw, C)
    g = _gen(seed)
    K = geom["KH"] * geom["KW"] * C
    x = _ints((geom["N"], geom["H"], geom["W"], C), 3, g)
    w = _ints((N, K), 7, g) * 2.0 ** -_k_shift(K)
    b = _ints((N,), 40, g) * 2.0 ** -_k_shift(K)
    return geom, x, w, b, gather_reference(x, w, geom, slice_major) + b


def _guarded_rows(v, lda, dtype):
    """[rows, C] values -> the [rows, C] view (row stride lda) into a NaN-filled buffer with GUARD NaN rows on either
    side and NaN in the columns C .. lda"""
    rows, C = v.shape
    full = torch.full((rows + 2 * GUARD, lda), float("nan"), dtype=dtype, device=DEV)
    full[GUARD:GUARD + rows, :C] = v.to(dtype).to(DEV)
    return full[GUARD:GUARD + rows, :C]


def _guarded_records(a_view):
    """fp32 [rows, C] -> its bf16x3 records inside a NaN-filled buffer: NaN records in front, NaN records behind, then
    the 256-byte zero page (skimi.h: "zero bytes that lie behind the records").  Returns the tensor ops.gemm takes as
    a_records: it begins at the first real record and ends with the zero page."""
    rows, C = a_view.shape
    rec = ops.split_records(a_view).reshape(-1)
    guard = GUARD * ((C + 31) // 32) * 64
    big = torch.full((guard + rec.numel() + guard + 128,), float("nan"), dtype=torch.bfloat16, device=DEV)
    big[guard:guard + rec.numel()] = rec
    big[-128:] = 0
    return big[guard:]


def check_exact(s, M, N, ldo, want, tol, geom, what):
    """every element of sentinel `s`: the [M, N] result (row stride ldo) against `want` (+- tol; 0 = equality), all
    others untouched.  A NaN or an unequal element is reported with the pixel it belongs to."""
    got, init = s.buf.double().cpu(), s.init.cpu()
    idx = (torch.arange(M)[:, None] * ldo + torch.arange(N)[None, :]).reshape(-1)
    keep = torch.ones(got.numel(), dtype=torch.bool)
    keep[idx] = False
    stray = keep & ~((got == init) | (torch.isnan(got) & torch.isnan(init)))
    assert not stray.any(), f"{what}: {int(stray.sum())} elements the descriptor does not address were written " \
                            f"(first at flat {int(stray.nonzero()[0])})"
    g = got[idx].view(M, N)
    bad = ~((g - want).abs() <= tol)   # a NaN is never within the bound
    if bad.any():
        i = int(bad.reshape(-1).nonzero()[0])
        m, n = divmod(i, N)
        where = f"row {m}, n {n}"
        if geom is not None:
            img, rem = divmod(m, geom["OH"] * geom["OW"])
            where = f"image {img}, oy {rem // geom['OW']}, ox {rem % geom['OW']}, n {n}"
        t = tol if isinstance(tol, (int, float)) else tol[m, n].item()
        raise AssertionError(f"{what}: {int(bad.sum())} of {M * N} elements off the float64 reference ({int(torch.isnan(g).sum())} "
                             f"NaN); first at flat {m * ldo + n} = ({where}): got {g[m, n].item()!r}, want "
                             f"{want[m, n].item()!r} +- {t:.3g}")


def run_gather(monkeypatch, *, name, size="small", C=None, N, pk="x3_a32", slice_major=False, lda_pad=None, x3=None,
               splitk=0, planes=None, env=None, expect, data="exact", seed=0, refused=False):
    """One gathered launch of ops.gemm (bias, fp32 out) against gather_reference.  name / size: the geometry and its
    image size ("small", "x3" or (n, H, W)); pk: a GEN_PRECS key; x3: None, or the A form of an LDS-DMA launch -- "fp32"
    (x3_scratch) or "records" (w_split either way); splitk: force_splitk over `planes` planes of scratch; refused: the
    launch must end in an argument error with no kernel chosen and no output element written."""
    _env(monkeypatch, env or {})
    prec, a_dt, w_dt = GEN_PRECS[pk]
    C = C or (128 if name in C128 else 64)
    lda = C + (LDA_PAD.get(name, 0) if lda_pad is None else lda_pad)
    if data == "exact":
        geom, x, w, b, want = _exact_case(name, _nhw(name, size), C, N, slice_major, seed)
        tol = 0.0
    else:   # random operands, rounded as the kernel rounds them; the error model of test_gemm_epilogue_gpu.run_case
        geom = make_geom(name, _nhw(name, size), C)
        g = _gen(seed)
        K = geom["KH"] * geom["KW"] * C
        x = torch.randn(geom["N"], geom["H"], geom["W"], C, generator=g, dtype=torch.float64).to(a_dt).double()
        w = (torch.randn(N, K, generator=g, dtype=torch.float64) / math.sqrt(K)).to(w_dt).double()
        b = (torch.rand(N, generator=g) * 2 - 1).double()
        if prec != PREC_BF16X3:
            x, w = x.to(H16[prec]).double(), w.to(H16[prec]).double()
        acc, mag = gather_reference(x, w, geom, slice_major), gather_reference(x.abs(), w.abs(), geom, slice_major)
        acc_err = ((2.0 ** -15 + K * U) if prec == PREC_BF16X3 else K * U) * mag
        want, tol = chain(acc, acc_err, bias=b)
    M, K = geom["N"] * geom["OH"] * geom["OW"], geom["KH"] * geom["KW"] * C
    rows = geom["N"] * geom["H"] * geom["W"]
    a_view = _guarded_rows(x.reshape(rows, C), lda, a_dt)
    w_t = w.to(w_dt).to(DEV)
    b_t = b.float().to(DEV)
    ldo = N + 4
    out_s = Sentinel(M * ldo + 8, torch.float32)
    kw = dict(conv=dict(geom, slice_major=slice_major))
    if x3 is not None:
        kw["w_split"] = ops.split_records(w_t)
        if x3 == "records":
            kw["a_records"] = _guarded_records(a_view)
        else:
            kw["x3_scratch"] = torch.full((ops.x3_scratch_numel(rows, C),), float("nan"), device=DEV)
    if splitk:
        kw["splitk_scratch"] = torch.full(((planes or splitk) * M * N,), float("nan"), device=DEV)
        kw["force_splitk"] = splitk
    launch = lambda: ops.gemm(None if x3 == "records" else a_view, w_t, prec=prec, bias=b_t, out=out_s.view(0, M, ldo, N), **kw)
    if refused:
        with pytest.raises(SkimiError):
            launch()
        assert ops.gemm_last_path().raw == 0
        torch.cuda.synchronize()
        assert torch.isnan(out_s.buf).all(), "a refused launch wrote output"
        return None
    launch()
    path = ops.gemm_last_path()
    torch.cuda.synchronize()
    for f_, v_ in expect.items():
        assert getattr(path, f_) == v_, f"dispatched to {path}, the case expects {f_} = {v_!r}"
    check_exact(out_s, M, N, ldo, want, tol, geom, f"{name} C={C} lda={lda} {pk}")
    if splitk:
        assert (kw["splitk_scratch"] == 0).all(), "split-K scratch not left zeroed"
    if x3 == "records":
        assert (kw["a_records"][-128:] == 0).all(), "the A records' zero page was written"
    return path


def _seed(*keys):
    return sum((i + 1) * 131 * (list(GEOMS).index(k) if k in GEOMS else int(k)) for i, k in enumerate(keys)) % 9973


# ---------------------------------------------------------------------------------------------------------------------
# generic kernel, 64x64 tile: every geometry x (prec, A dtype); slice-major under bf16x3
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("pk", list(GEN_PRECS))
@pytest.mark.parametrize("name", list(GEOMS))
def test_generic_64(name, pk, monkeypatch):
    run_gather(monkeypatch, name=name, N=100, pk=pk, seed=_seed(name, 1),
               expect=dict(family="generic", tile="64x64", splitk=1))


@gpu
@pytest.mark.parametrize("pk", ["x3_a32", "x3_a16"])
@pytest.mark.parametrize("name", list(GEOMS))
def test_generic_64_slice_major(name, pk, monkeypatch):
    """a_mode 2 on three 32-channel slices"""
    run_gather(monkeypatch, name=name, C=96, N=100, pk=pk, slice_major=True, seed=_seed(name, 2),
               expect=dict(family="generic", tile="64x64", splitk=1))


# ---------------------------------------------------------------------------------------------------------------------
# generic kernel, 128x64 and 128x128 tiles: one (prec, A dtype) per mode
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("pk", ["x3_a32", "bf16_a16", "f16_a32"])
@pytest.mark.parametrize("name", ["same3", "s2", "dil2", "rect"])
@pytest.mark.parametrize("tile", list(BIG))
def test_generic_large_tiles(tile, name, pk, monkeypatch):
    N, sizes = BIG[tile]
    run_gather(monkeypatch, name=name, size=sizes[name], N=N, pk=pk, seed=_seed(name, 3 + list(BIG).index(tile)),
               expect=dict(family="generic", tile=tile, splitk=1))


# ---------------------------------------------------------------------------------------------------------------------
# split-K with a gather: a split starts in the middle of the tap sequence.  (geometry, cC, precision, slice-major, where the
# split boundaries fall): "between" two taps, "inside" a tap's channel range (tap-major), or in the "middle" of a
# slice's taps (slice-major)
# ---------------------------------------------------------------------------------------------------------------------
SPLITK = [("same3", 64, "x3_a32", False, "between"), ("same3", 64, "bf16_a16", False, "between"),
          ("dil2", 64, "f16_a32", False, "between"), ("dil2", 96, "x3_a16", True, "between"),
          ("vp3d_k3d9", 64, "bf16_a32", False, "between"), ("vp3d_k5d3", 128, "x3_a32", False, "inside"),
          ("vp3d_k5d3", 128, "x3_a16", True, "middle"), ("vp3d_k5d3", 128, "f16_a16", False, "between")]


def _cdiv(a, b):
    return -(-a // b)


def _split_boundary(name, C, pk, slice_major):
    """where gemm_dispatch's split of K in three puts the boundaries (k_per_split = cdiv(cdiv(K, BK), 3) * BK)"""
    KH, KW = GEOMS[name][0][:2]
    BK = 32 if GEN_PRECS[pk][0] == PREC_BF16X3 else 64
    K = KH * KW * C
    kper = _cdiv(_cdiv(K, BK), 3) * BK
    assert _cdiv(K, kper) == 3
    if slice_major:
        return "between" if (kper // 32) % (KH * KW) == 0 else "middle"
    return "between" if kper % C == 0 else "inside"


def test_splitk_cases_cover_both_boundaries():
    for name, C, pk, sm, where in SPLITK:
        assert _split_boundary(name, C, pk, sm) == where, (name, C, pk)
    assert {"between", "inside", "middle"} == {c[4] for c in SPLITK}


@gpu
@pytest.mark.parametrize("mode", ["ordered", "atomic"])
@pytest.mark.parametrize("name,C,pk,slice_major,where", SPLITK)
def test_splitk(name, C, pk, slice_major, where, mode, monkeypatch):
    run_gather(monkeypatch, name=name, C=C, N=100, pk=pk, slice_major=slice_major, splitk=3,
               planes=3 if mode == "ordered" else 1, seed=_seed(name, 5),
               expect=dict(family="splitk_" + mode, tile="64x64", splitk=3))


# ---------------------------------------------------------------------------------------------------------------------
# LDS-DMA bf16x3 kernels (SKIMI_X3_MIN_TILES=1): wide (N > 128) and narrow loop x MFMA shape x a_mode x every geometry
# but k6; the A form (fp32 split into records first / records given) alternates so that each (loop, geometry) and each
# (loop, MFMA shape, a_mode) meets both
# ---------------------------------------------------------------------------------------------------------------------
X3_N = {"wide": 352, "narrow": 128}   # 352: a ragged second column tile; the narrow loop's ragged N: 100 on dil2


def _x3_cases():
    return [(kind, mfma, mode, name) for kind in X3_N for mfma in (16, 32) for mode in (1, 2) for name in X3_GEOMS]


@gpu
@pytest.mark.parametrize("kind,mfma,mode,name", _x3_cases())
def test_x3dma(kind, mfma, mode, name, monkeypatch):
    form = ("fp32", "records")[(X3_GEOMS.index(name) + mfma // 32 + mode) % 2]
    N = 100 if (kind, name) == ("narrow", "dil2") else X3_N[kind]
    run_gather(monkeypatch, name=name, size="x3", C=96 if mode == 2 else None, N=N, slice_major=mode == 2, x3=form,
               env={"SKIMI_X3_MIN_TILES": 1, "SKIMI_X3_MFMA": mfma}, seed=_seed(name, 6 + mode),
               expect=dict(family="x3dma_" + kind, mfma=mfma, splitk=1))


@gpu
@pytest.mark.parametrize("form", ["fp32", "records"])
@pytest.mark.parametrize("N", [128, 352])
def test_x3dma_declines_36_taps(N, form, monkeypatch):
    """KH * KW > 32 does not fit the LDS-DMA kernels' tap mask: fp32 A goes to the generic kernel and is exact; A records,
    which only those kernels read, are refused and nothing is written"""
    env = {"SKIMI_X3_MIN_TILES": 1}
    if form == "fp32":
        run_gather(monkeypatch, name="k6", size="x3", N=N, x3="fp32", env=env, seed=_seed("k6", 8),
                   expect=dict(family="generic", tile="64x64", splitk=1))
    else:
        run_gather(monkeypatch, name="k6", size="x3", N=N, x3="records", env=env, seed=_seed("k6", 8), expect={}, refused=True)


@gpu
@pytest.mark.parametrize("form", ["fp32", "records"])
@pytest.mark.parametrize("N", [128, 352])
def test_x3dma_tap_behind_the_input(N, form, monkeypatch):
    """dil2 on ONE image of two rows: the window's last tap (dy = 4, dx = 4 against pad 2) starts behind the whole input,
    all its lanes are padding.  The LDS-DMA kernels reach the zero page as an unsigned offset from that tap's base, so
    the base has to lie in front of it: with fp32 A the zero page follows the records at once and gemm_x3dma_eligible
    hands the launch to the generic kernel; with records whose zero page lies GUARD pixels further back the base is in
    front of it and the LDS-DMA kernel serves the launch.  Exact either way."""
    kind = "narrow" if N <= 128 else "wide"
    expect = dict(family="generic", tile="64x64", splitk=1) if form == "fp32" else dict(family="x3dma_" + kind, splitk=1)
    run_gather(monkeypatch, name="dil2", size=(1, 2, 160), N=N, x3=form, env={"SKIMI_X3_MIN_TILES": 1},
               seed=_seed("dil2", 10), expect=expect)


# ---------------------------------------------------------------------------------------------------------------------
# conv_win (SKIMI_CONV_WIN=2): its window loads with NaN around the images and a pixel stride lda > cC
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("pk", ["bf16_a16", "f16_a16"])
def test_conv_win(pk, C, monkeypatch):
    """three images of 20 x 23: ragged 16 x 16 pixel tiles on both axes, halo rows that belong to the neighbouring image"""
    run_gather(monkeypatch, name="same3", size=(3, 20, 23), C=C, N=128, pk=pk, lda_pad=8, env={"SKIMI_CONV_WIN": 2},
               seed=_seed("same3", 9), expect=dict(family="conv_win", splitk=1))


# ---------------------------------------------------------------------------------------------------------------------
# random data, one case per kernel family: the contraction against the precision's error model
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("family", ["generic", "splitk_ordered", "x3dma_wide", "x3dma_narrow", "conv_win"])
def test_random_data(family, monkeypatch):
    c = {"generic": dict(name="dil2", N=100, pk="bf16_a32", expect=dict(family="generic", tile="64x64")),
         "splitk_ordered": dict(name="vp3d_k5d3", C=128, N=100, splitk=3, expect=dict(family="splitk_ordered", splitk=3)),
         "x3dma_wide": dict(name="k5", size="x3", N=352, x3="fp32", env={"SKIMI_X3_MIN_TILES": 1},
                            expect=dict(family="x3dma_wide")),
         "x3dma_narrow": dict(name="dil2", size="x3", C=96, N=128, slice_major=True, x3="records",
                              env={"SKIMI_X3_MIN_TILES": 1}, expect=dict(family="x3dma_narrow")),
         "conv_win": dict(name="same3", size=(3, 20, 23), N=128, pk="f16_a16", lda_pad=8, env={"SKIMI_CONV_WIN": 2},
                          expect=dict(family="conv_win"))}[family]
    run_gather(monkeypatch, **c, data="random", seed=21)


# ---------------------------------------------------------------------------------------------------------------------
# plain rows (a_mode 0): lda > K with NaN in the padding, K % 8 == 0 but no multiple of the K-tile
# ---------------------------------------------------------------------------------------------------------------------
def run_rows(monkeypatch, *, M, N, K, pk="x3_a32", x3=None, splitk=0, planes=None, env=None, expect, seed=0):
    _env(monkeypatch, env or {})
    prec, a_dt, w_dt = GEN_PRECS[pk]
    g = _gen(seed)
    a = _ints((M, K), 3, g)
    w = _ints((N, K), 7, g) * 2.0 ** -_k_shift(K)
    b = _ints((N,), 40, g) * 2.0 ** -_k_shift(K)
    want = a @ w.T + b
    a_view = _guarded_rows(a, K + 8, a_dt)
    w_t, b_t = w.to(w_dt).to(DEV), b.float().to(DEV)
    ldo = N + 4
    out_s = Sentinel(M * ldo + 8, torch.float32)
    kw = {}
    if x3 is not None:
        kw["w_split"] = ops.split_records(w_t)
        if x3 == "records":
            kw.update(a_records=_guarded_records(a_view), M=M, lda=K)
        else:
            kw["x3_scratch"] = torch.full((ops.x3_scratch_numel(M, K),), float("nan"), device=DEV)
    if splitk:
        kw["splitk_scratch"] = torch.full(((planes or splitk) * M * N,), float("nan"), device=DEV)
        kw["force_splitk"] = splitk
    ops.gemm(None if x3 == "records" else a_view, w_t, prec=prec, bias=b_t, out=out_s.view(0, M, ldo, N), **kw)
    path = ops.gemm_last_path()
    torch.cuda.synchronize()
    for f_, v_ in expect.items():
        assert getattr(path, f_) == v_, f"dispatched to {path}, the case expects {f_} = {v_!r}"
    check_exact(out_s, M, N, ldo, want, 0.0, None, f"rows K={K} lda={K + 8} {pk}")
    if splitk:
        assert (kw["splitk_scratch"] == 0).all(), "split-K scratch not left zeroed"


@gpu
@pytest.mark.parametrize("pk", list(GEN_PRECS))
def test_rows_generic(pk, monkeypatch):
    run_rows(monkeypatch, M=300, N=100, K=136, pk=pk, seed=31, expect=dict(family="generic", tile="64x64", splitk=1))


@gpu
@pytest.mark.parametrize("mode", ["ordered", "atomic"])
@pytest.mark.parametrize("pk", ["x3_a32", "bf16_a16", "f16_a32"])
def test_rows_splitk(pk, mode, monkeypatch):
    run_rows(monkeypatch, M=300, N=100, K=136, pk=pk, splitk=3, planes=3 if mode == "ordered" else 1, seed=32,
             expect=dict(family="splitk_" + mode, splitk=3))


@gpu
@pytest.mark.parametrize("form", ["fp32", "records"])
@pytest.mark.parametrize("mfma", [16, 32])
@pytest.mark.parametrize("kind", list(X3_N))
def test_rows_x3dma(kind, mfma, form, monkeypatch):
    run_rows(monkeypatch, M=612, N=X3_N[kind], K=136, x3=form, env={"SKIMI_X3_MIN_TILES": 1, "SKIMI_X3_MFMA": mfma},
             seed=33, expect=dict(family="x3dma_" + kind, mfma=mfma, splitk=1))


@gpu
@pytest.mark.parametrize("pk", ["bf16_a16", "f16_a16"])
def test_rows_gemm256(pk, monkeypatch):
    """gemm256_eligible takes K % 64 == 0 only: the padded row stride is what this case adds"""
    run_rows(monkeypatch, M=2300, N=520, K=192, pk=pk, seed=34, expect=dict(family="gemm256", splitk=1))


# ---------------------------------------------------------------------------------------------------------------------
# refusals: an argument error, no kernel chosen and no output element written
# ---------------------------------------------------------------------------------------------------------------------
def _refused(monkeypatch, *, name="same3", C=64, pk="x3_a32", K_extra=0, lda=None, M=None, conv_fix=None):
    _env(monkeypatch, {})
    prec, a_dt, w_dt = GEN_PRECS[pk]
    geom = make_geom(name, _nhw(name, "small"), C)
    geom.update(conv_fix or {})
    rows, K = geom["N"] * geom["H"] * geom["W"], geom["KH"] * geom["KW"] * C + K_extra
    g = _gen(41)
    a_view = _guarded_rows(_ints((rows, C), 3, g), C + 8, a_dt)
    w_t = _ints((100, K), 7, g).to(w_dt).to(DEV)
    out_rows = max(M or 0, geom["N"] * geom["OH"] * geom["OW"])
    out = torch.full((out_rows, 100), float("nan"), device=DEV)
    with pytest.raises(SkimiError):
        ops.gemm(a_view, w_t, prec=prec, out=out, conv=geom, M=M, lda=lda)
    assert ops.gemm_last_path().raw == 0
    torch.cuda.synchronize()
    assert torch.isnan(out).all(), "a refused launch wrote output"


@gpu
@pytest.mark.parametrize("what", ["K", "M", "window", "cC_x3", "cC_bf16", "lda"])
def test_refusals(what, monkeypatch):
    _refused(monkeypatch, **{"K": dict(K_extra=64),                       # K != KH*KW*cC
                             "M": dict(M=3 * 7 * 9 + 1),                  # M != cN*OH*OW
                             "window": dict(conv_fix=dict(OH=8)),         # the last window starts below cH + pad
                             "cC_x3": dict(C=48),                         # cC % 32 != 0
                             "cC_bf16": dict(C=96, pk="bf16_a16"),        # cC % 64 != 0 on 16-bit operands
                             "lda": dict(lda=56)}[what])                  # pixel stride < cC
