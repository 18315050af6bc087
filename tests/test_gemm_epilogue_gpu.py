"""The fused GEMM epilogue (skimi_gemm_desc, include/skimi.h) on every kernel that runs it, against a float64 reference.

The epilogue exists in five copies: the shared store_one / store_four (generic kernel, split-K second pass, conv_win,
gemm256 EPI 0), gemm256's compile-time EPI 1 / 2 / 3 (interior and edge tiles) and the x3dma fast path (wide and
narrow).  Every GPU case here
  * pins the kernel it means: ops.gemm_last_path() must name the family, tile / loop, MFMA shape, EPI kind and split
    count of the case before any value is looked at;
  * uses operands that make the contraction exact (small integers in A, integers * 2^-k in W: exact in bf16, fp16 and
    bf16x3, and every fp32 partial sum is exact), so the only error left is the epilogue's fp32 rounding, the
    activation's approximation and the output rounding -- bounded per element by `chain` below, never by a norm;
  * fills out, out2 and the records with NaN first: what the descriptor does not address must still be NaN after the
    launch (rows skipped by out_row_off, columns between N and ldo, batch gaps of out_batch_stride), and the records'
    256-byte zero page must be zero.
One random-data case per family checks the contraction itself against the precision's error model.

`reference` knows nothing about kernels: it is the descriptor's documented semantics, pinned on the CPU against torch
compositions (test_reference_matches_torch_compositions)."""
import math

import pytest
import torch
import torch.nn.functional as F

from skiing_analysis_pytorch_amd import ops
from skiing_analysis_pytorch_amd._lib import (ACT_GELU, ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_SILU, PREC_BF16,
                                              PREC_BF16X3, PREC_F16)

DEV = "cuda"
U = 2.0 ** -24   # fp32 unit roundoff
ACTS = [ACT_NONE, ACT_RELU, ACT_GELU, ACT_SILU, ACT_SIGMOID]
H16 = {PREC_BF16: torch.bfloat16, PREC_BF16X3: torch.bfloat16, PREC_F16: torch.float16}   # the mode's 16-bit format


# ---------------------------------------------------------------------------------------------------------------------
# float64 reference of the descriptor (skimi.h: "epilogue: v = acc + bias[n]; v = act(v); v *= gamma[n];
# v += resid[m', n]; ... v += resid2[m, n]; v = post_act(v)", then the store)
# ---------------------------------------------------------------------------------------------------------------------
def act64(v, act):
    if act == ACT_NONE:
        return v
    if act == ACT_RELU:
        return v.clamp_min(0.0)
    if act == ACT_GELU:
        return 0.5 * v * (1.0 + torch.erf(v / math.sqrt(2.0)))
    if act == ACT_SILU:
        return v / (1.0 + torch.exp(-v))
    if act == ACT_SIGMOID:
        return 1.0 / (1.0 + torch.exp(-v))
    raise ValueError(act)


def row_map(m, rows_per_batch, batch_stride, row_off):
    """skimi.h's row remap: (m / rpb) * batch_stride + m % rpb + row_off (rpb 0 = m + row_off)"""
    if rows_per_batch > 0:
        return (m // rows_per_batch) * batch_stride + m % rows_per_batch + row_off
    return m + row_off


def reference(acc, *, bias=None, act=ACT_NONE, gamma=None, resid=None, resid_map=None, resid2=None,
              post_act=ACT_NONE):
    """acc [M, N] float64 -> the epilogue's value of every (m, n), float64.  resid [rows, >= N] is read at row m'
    (resid_map = (rows_per_batch, batch_stride, row_off)), resid2 [>= M, >= N] at row m."""
    M, N = acc.shape
    v = acc.double()
    if bias is not None:
        v = v + bias.double()
    v = act64(v, act)
    if gamma is not None:
        v = v * gamma.double()
    if resid is not None:
        rows = row_map(torch.arange(M, device=acc.device), *(resid_map or (0, 0, 0)))
        v = v + resid.double()[rows, :N]
    if resid2 is not None:
        v = v + resid2.double()[:M, :N]
    return act64(v, post_act)


def store_index(M, N, ldo, *, out_map=None, pixel_shuffle=None):
    """[M, N] element offsets of the store: out_map = (rows_per_batch, batch_stride, row_off) for store_mode 0,
    pixel_shuffle = (s, Cout, cN, cH, cW) for store_mode 1 (ConvTranspose2d with kernel == stride)"""
    m = torch.arange(M).unsqueeze(1)
    n = torch.arange(N).unsqueeze(0)
    if pixel_shuffle is None:
        return row_map(m, *(out_map or (0, 0, 0))) * ldo + n
    s, cout, _, cH, cW = pixel_shuffle
    img, rem = m // (cH * cW), m % (cH * cW)
    iy, ix = rem // cW, rem % cW
    ab, co = n // cout, n % cout
    a, b = ab // s, ab % s
    return ((img * cH * s + iy * s + a) * (cW * s) + ix * s + b) * ldo + co


# ---- error model of the kernels' epilogue (gemm_epilogue.h) ----
LIPSCHITZ = {ACT_NONE: 1.0, ACT_RELU: 1.0, ACT_GELU: 1.13, ACT_SILU: 1.1, ACT_SIGMOID: 0.25}


def act_err(x, act):
    """|kernel act(x) - act(x)| for an fp32 input x, the result's own rounding included.
    GELU: erfc by Abramowitz & Stegun 7.1.26 (|error| <= 1.5e-7, times |x| / 2), its polynomial in fp32 (coefficient
    sum 4.5 against a value >= 1: <= 23 ulp of q) plus hardware rcp / exp2 (1 ulp each) and the rounded exp2 argument
    (~0.4 x^2 ulp of q, and q x^2 <= 0.5): <= |x| (0.75e-7 + 32 u) + u |gelu|.
    sigmoid = rcp(1 + exp2(-log2(e) x)): the rounded product moves exp by |x| u, the constant by |x| u more, exp2 and rcp
    are 1 ulp (2 u) each, the add 1 u: relative (2 |x| + 6) u.  SiLU = x * sigmoid: one rounding more."""
    a = x.abs()
    if act in (ACT_NONE, ACT_RELU):
        return torch.zeros_like(a)
    y = act64(x, act).abs()
    if act == ACT_GELU:
        return a * (0.75e-7 + 32 * U) + U * y
    if act == ACT_SIGMOID:
        return y * (2 * a + 6) * U
    return y * (2 * a + 7) * U


def chain(acc, acc_err, *, bias=None, act=ACT_NONE, gamma=None, resid=None, resid_map=None, resid2=None,
          post_act=ACT_NONE):
    """(value, error bound) of the fp32 epilogue, step by step as reference() computes it: one fp32 rounding per add /
    multiply (u times the magnitude of its exact result), the activations' bounds, and the Lipschitz constants of the
    activations for the error that flows through them.  The bound is doubled: the rounding points are the computed
    (not the exact) intermediates."""
    M, N = acc.shape
    v, e = acc.double(), acc_err.double()
    if bias is not None:
        v = v + bias.double()
        e = e + U * v.abs()
    e = LIPSCHITZ[act] * e + act_err(v, act)
    v = act64(v, act)
    if gamma is not None:
        g = gamma.double()
        v = v * g
        e = e * g.abs() + U * v.abs()
    if resid is not None:
        rows = row_map(torch.arange(M, device=acc.device), *(resid_map or (0, 0, 0)))
        v = v + resid.double()[rows, :N]
        e = e + U * v.abs()
    if resid2 is not None:
        v = v + resid2.double()[:M, :N]
        e = e + U * v.abs()
    e = LIPSCHITZ[post_act] * e + act_err(v, post_act)
    return act64(v, post_act), 2 * e


def ulp(x, dtype):
    """one ulp of `dtype` at |x| (float64 tensor)"""
    mant, emin = {torch.float32: (23, -126), torch.bfloat16: (7, -126), torch.float16: (10, -14)}[dtype]
    e = torch.floor(torch.log2(x.abs().clamp_min(2.0 ** emin)))
    return torch.pow(2.0, e - mant)


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the reference itself, against torch compositions
# ---------------------------------------------------------------------------------------------------------------------
def test_reference_matches_torch_compositions():
    g = torch.Generator().manual_seed(5)
    M, N, K = 23, 13, 16
    a = torch.randn(M, K, generator=g, dtype=torch.float64)
    w = torch.randn(N, K, generator=g, dtype=torch.float64)
    b = torch.randn(N, generator=g, dtype=torch.float64)
    gm = torch.randn(N, generator=g, dtype=torch.float64)
    r = torch.randn(40, N + 3, generator=g, dtype=torch.float64)
    r2 = torch.randn(M, N + 5, generator=g, dtype=torch.float64)
    acc = a @ w.T
    torch_act = {ACT_NONE: lambda x: x, ACT_RELU: F.relu, ACT_GELU: F.gelu, ACT_SILU: F.silu, ACT_SIGMOID: torch.sigmoid}
    for act in ACTS:
        for post in (ACT_NONE, ACT_RELU, ACT_SIGMOID):
            rm = (5, 8, 2)   # rows 2..6 of each batch of 8
            rows = [(m // 5) * 8 + m % 5 + 2 for m in range(M)]
            want = torch_act[post](torch_act[act](F.linear(a, w, b)) * gm + r[rows, :N] + r2[:, :N])
            got = reference(acc, bias=b, act=act, gamma=gm, resid=r, resid_map=rm, resid2=r2, post_act=post)
            assert torch.allclose(got, want, rtol=1e-12, atol=1e-12), (act, post)
            # the GPU cases take value and bound from chain(): its value is reference()'s
            val, _ = chain(acc, torch.zeros_like(acc), bias=b, act=act, gamma=gm, resid=r, resid_map=rm, resid2=r2,
                           post_act=post)
            assert torch.equal(val, got)
    # broadcast over frames (batch stride 0) and a plain offset
    got = reference(acc, resid=r, resid_map=(7, 0, 1))
    assert torch.allclose(got, acc + r[[1 + m % 7 for m in range(M)], :N])
    got = reference(acc, resid=r, resid_map=(0, 0, 3))
    assert torch.allclose(got, acc + r[3:3 + M, :N])
    # stores: output row remap, and the pixel shuffle of ConvTranspose2d(k == s) against torch
    idx = store_index(6, 4, 10, out_map=(2, 5, 1))
    assert idx[0].tolist() == [10, 11, 12, 13] and idx[1, 0] == 20 and idx[2, 0] == 60 and idx[5, 3] == 123
    s, cout, cN, cH, cW = 2, 3, 2, 3, 4
    x = torch.randn(cN, 5, cH, cW, generator=g, dtype=torch.float64)
    wt = torch.randn(5, cout, s, s, generator=g, dtype=torch.float64)
    want = F.conv_transpose2d(x, wt, stride=s).permute(0, 2, 3, 1)           # [cN, cH s, cW s, cout]
    wmat = wt.permute(2, 3, 1, 0).reshape(s * s * cout, 5)                     # n = (a s + b) Cout + co
    val = x.permute(0, 2, 3, 1).reshape(-1, 5) @ wmat.T
    out = torch.full((want.numel(),), float("nan"), dtype=torch.float64)
    out[store_index(cN * cH * cW, s * s * cout, cout, pixel_shuffle=(s, cout, cN, cH, cW)).reshape(-1)] = val.reshape(-1)
    assert torch.allclose(out.view_as(want), want)
    # the error model covers fp32 evaluations of the same activations (torch's fp32 kernels)
    x = torch.linspace(-9, 9, 4001, dtype=torch.float64)
    for act, f in ((ACT_GELU, F.gelu), (ACT_SILU, F.silu), (ACT_SIGMOID, torch.sigmoid)):
        assert ((f(x.float()).double() - act64(x, act)).abs() <= act_err(x, act)).all(), act


def test_activation_bounds_cover_the_kernel_formulas():
    """the kernels' own formulas (gemm_epilogue.h: gelu_erf, gelu_erf2, sigmoid_hw), evaluated step by step in fp32 with
    correctly rounded exp2 / reciprocal (the hardware's are within 1 ulp, which act_err allows for twice over)"""
    x = torch.linspace(-10, 10, 20001, dtype=torch.float32)
    f32 = lambda t: t.float()
    z = f32(x.abs() * 0.70710678118654752440)
    t = f32(1.0 / f32(0.3275911 * z + 1.0))
    q = f32(t * 1.061405429 - 1.453152027)
    q = f32(t * q + 1.421413741)
    q = f32(t * q - 0.284496736)
    q = f32(t * q + 0.254829592)
    q = f32(f32(f32(q * t) * f32(torch.exp2(f32(f32(-1.4426950408889634 * z) * z)))) * 0.5)
    gelu = torch.where(x >= 0, f32(x - x * q), f32(x * q))
    sig = f32(1.0 / f32(1.0 + f32(torch.exp2(f32(-1.4426950408889634 * x)))))
    silu = f32(x * sig)
    x64 = x.double()
    for act, y in ((ACT_GELU, gelu), (ACT_SIGMOID, sig), (ACT_SILU, silu)):
        err = (y.double() - act64(x64, act)).abs()
        assert (err <= act_err(x64, act) / 2).all(), (act, (err / act_err(x64, act)).max().item())


# ---------------------------------------------------------------------------------------------------------------------
# GPU harness
# ---------------------------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _ints(shape, lim, g):
    return torch.randint(-lim, lim + 1, shape, generator=g).double()


def _k_shift(K):
    """W = integers * 2^-k with k such that the exact accumulators spread over about [-6, 6] (std ~ 3)"""
    return max(0, round(math.log2(math.sqrt(K * 4.0 * 18.7) / 3.0)))


def _padded(rows, cols, ld, dtype, g, scale=1.0, exact16=None):
    """[rows, ld] buffer of random values, returned as the [rows, cols] view (row stride ld) and its float64 values.
    exact16: values exactly representable in that 16-bit format"""
    full = torch.randn(rows, ld, generator=g) * scale
    if exact16 is not None:
        full = full.to(exact16).float()
    t = full.to(dtype).to(DEV)
    return t[:, :cols], t.double()


class Sentinel:
    """a buffer behind a strided view (NaN-filled, or given: the residual an in-place launch overwrites); `check`
    compares every element of the whole buffer -- addressed elements against value +- tol, all others against the
    buffer's content before the launch"""

    def __init__(self, numel=0, dtype=torch.float32, wrap=None):
        self.buf = torch.full((numel,), float("nan"), dtype=dtype, device=DEV) if wrap is None else wrap
        self.init = self.buf.double().clone()

    def view(self, off, rows, ld, cols):
        return self.buf[off:off + rows * ld].view(rows, ld)[:, :cols]

    def check(self, idx, value, tol, what):
        flat = idx.reshape(-1).to(DEV)
        got = self.buf.double()
        want = self.init.clone()
        want[flat] = value.reshape(-1)
        t = torch.zeros_like(want)
        t[flat] = tol.reshape(-1)
        addressed = torch.zeros_like(want, dtype=torch.bool)
        addressed[flat] = True
        keep = ~addressed
        same = (got == want) | (torch.isnan(got) & torch.isnan(want))
        stray = keep & ~same
        assert not stray.any(), f"{what}: {int(stray.sum())} elements the descriptor does not address were written " \
                                f"(first at flat {int(stray.nonzero()[0])})"
        bad = addressed & ~((got - want).abs() <= t)
        if bad.any():
            i = int(bad.nonzero()[0])
            raise AssertionError(f"{what}: {int(bad.sum())} of {int(addressed.sum())} elements outside the bound; first "
                                 f"at flat {i}: got {got[i].item()!r}, want {want[i].item()!r} +- {t[i].item():.3g}")


def _env(monkeypatch, env):
    for k in ("SKIMI_GEMM256_MT3", "SKIMI_GEMM256_W4", "SKIMI_GEMM256_PP", "SKIMI_GEMM256_MFMA", "SKIMI_X3_MIN_TILES",
              "SKIMI_CONV_WIN"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))


def run_case(monkeypatch, *, M=None, N, K=None, prec=PREC_BF16X3, a_dt=torch.float32, w_dt=torch.float32, data="exact",
             bias=False, gamma=False, act=ACT_NONE, resid=None, resid_map=None, resid2=False, post_act=ACT_NONE,
             out_dt=torch.float32, out_map=None, out2=False, ldo_pad=0, out_off=0, records=False, conv=None,
             pixel_shuffle=None, w_split=False, a_records=False, splitk=0, splitk_planes=None, inplace=False, env=None,
             expect=None, seed=0, resid_rows=0):
    """One launch of ops.gemm with the given descriptor features, checked against reference() with sentinels.
    resid: None or the residual dtype (resid2 shares it: fp32 without resid); resid_map (rpb, batch_stride, row_off),
    out_map likewise for the output rows; out_dt None: records only; conv: dict(N, H, W, C, KH, KW, stride, pad)
    (implicit im2col, tap-major K); splitk: force_splitk over splitk_planes planes of scratch; inplace: out is resid
    (EPI 2); expect: fields of ops.gemm_last_path() the launch must report."""
    _env(monkeypatch, env or {})
    g = _gen(seed)
    # ---- operands ----
    cv = None
    a_shape = (M, K)
    if conv is not None:
        cv = dict(conv, dil=1)
        cv["OH"] = (cv["H"] + 2 * cv["pad"] - (cv["KH"] - 1) - 1) // cv["stride"] + 1
        cv["OW"] = (cv["W"] + 2 * cv["pad"] - (cv["KW"] - 1) - 1) // cv["stride"] + 1
        M = cv["N"] * cv["OH"] * cv["OW"]
        K = cv["KH"] * cv["KW"] * cv["C"]
        a_shape = (cv["N"] * cv["H"] * cv["W"], cv["C"])
    if data == "exact":
        a64 = _ints(a_shape, 3, g)
        w64 = _ints((N, K), 7, g) * 2.0 ** -_k_shift(K)
    else:
        a64 = torch.randn(a_shape, generator=g, dtype=torch.float64)
        w64 = torch.randn((N, K), generator=g, dtype=torch.float64) / math.sqrt(K)
    a_t = a64.to(a_dt).to(DEV)
    w_t = w64.to(w_dt).to(DEV)
    # what the MFMA multiplies: operands rounded to the mode's 16-bit format (bf16x3: the fp32 values)
    if prec == PREC_BF16X3:
        a_op, w_op = a_t.double(), w_t.double()
    else:
        a_op, w_op = a_t.to(H16[prec]).double(), w_t.to(H16[prec]).double()
    if cv is not None:
        def conv2d(x, w):
            x = x.view(cv["N"], cv["H"], cv["W"], cv["C"]).permute(0, 3, 1, 2)
            w = w.view(N, cv["KH"], cv["KW"], cv["C"]).permute(0, 3, 1, 2)
            return F.conv2d(x, w, stride=cv["stride"], padding=cv["pad"]).permute(0, 2, 3, 1).reshape(M, N)
        acc, mag = conv2d(a_op, w_op), conv2d(a_op.abs(), w_op.abs())
    else:
        acc, mag = a_op @ w_op.T, a_op.abs() @ w_op.abs().T
    if data == "exact":
        acc_err = torch.zeros_like(acc)
    elif prec == PREC_BF16X3:   # dropped lo * lo term (2^-16) and the lo halves' own rounding (2 x 2^-17), fp32 sums
        acc_err = (2.0 ** -15 + K * U) * mag
    else:                       # operands pre-rounded above: fp32 accumulation only
        acc_err = K * U * mag
    # ---- epilogue operands ----
    b = (torch.rand(N, generator=g) * 2 - 1).to(DEV) if bias else None
    gm = (torch.rand(N, generator=g) + 0.5).to(DEV) if gamma else None
    r_dt = resid if resid is not None else torch.float32
    ex16 = r_dt if r_dt != torch.float32 else None
    r_view = r2_view = None
    if resid is not None:
        rows = int(row_map(torch.arange(M), *(resid_map or (0, 0, 0))).max()) + 1
        ldr = N if inplace else N + 4
        r_view, _ = _padded(max(rows + 3, resid_rows), N, ldr, r_dt, g, scale=2.0, exact16=ex16)
    if resid2:   # a row stride of its own (ldr2 != ldr)
        r2_view, _ = _padded(M, N, N + 12 if N % 4 == 0 else N + 5, r_dt, g, scale=2.0, exact16=ex16)
    # ---- outputs (NaN sentinels) ----
    ldo = N + ldo_pad
    out_rows = int(row_map(torch.arange(M), *out_map).max()) + 3 if out_map is not None else M
    if pixel_shuffle is not None:
        s_, cout, n_img, h_, w_ = pixel_shuffle
        out_rows, cols = n_img * h_ * s_ * w_ * s_, cout
    else:
        cols = N
    out_s = out_t = None
    if inplace:
        assert resid_map is None and r_view.is_contiguous()
        out_s = Sentinel(wrap=r_view.view(-1))
        out_t = r_view[:M]
    elif out_dt is not None:
        out_s = Sentinel(out_rows * ldo + out_off + 7, out_dt)
        out_t = out_s.view(out_off, out_rows, ldo, cols)
    out2_s = out2_t = None
    if out2:
        out2_s = Sentinel(out_rows * (ldo + 8) + 5, torch.bfloat16 if out_dt == torch.float32 else torch.float32)
        out2_t = out2_s.view(0, out_rows, ldo + 8, cols)
    rec = None
    if records:
        rec = ops.records_buffer(M, N)
        rec.fill_(float("nan"))
    # ---- kernel-specific operands ----
    kw = {}
    if w_split:
        kw["w_split"] = ops.split_records(w_t)
        if a_records:
            ar = ops.records_buffer(*a_shape)
            ar.fill_(float("nan"))
            nrec = a_shape[0] * ((a_shape[1] + 31) // 32) * 64
            ar[:nrec] = ops.split_records(a_t).reshape(-1)
            ar[nrec:] = 0
            kw.update(a_records=ar, M=M, lda=K)
        else:
            kw["x3_scratch"] = torch.empty(ops.x3_scratch_numel(*a_shape), dtype=torch.float32, device=DEV)
    if splitk:
        kw["splitk_scratch"] = torch.full(((splitk_planes or splitk) * M * N,), float("nan"), device=DEV)
        kw["force_splitk"] = splitk
    if cv is not None:
        kw["conv"] = cv
    if pixel_shuffle is not None:
        kw["pixel_shuffle"] = pixel_shuffle
    # ---- reference (before the launch: in place, out is resid) ----
    val, err = chain(acc, acc_err, bias=b, act=act, gamma=gm, resid=r_view, resid_map=resid_map, resid2=r2_view,
                     post_act=post_act)
    ops.gemm(None if a_records else a_t, w_t, prec=prec, bias=b, gamma=gm, resid=r_view, act=act, out=out_t,
             out_dtype=out_dt or torch.float32, resid_map=resid_map, post_act=post_act, resid2=r2_view, out2=out2_t,
             out_map=out_map, out_records=rec, records_only=out_t is None, **kw)
    path = ops.gemm_last_path()
    torch.cuda.synchronize()
    for f_, v_ in (expect or {}).items():
        assert getattr(path, f_) == v_, f"dispatched to {path}, the case expects {f_} = {v_!r}"
    # ---- checks ----
    if out_t is not None:
        idx = store_index(M, N, ldo, out_map=out_map, pixel_shuffle=pixel_shuffle) + (0 if inplace else out_off)
        out_s.check(idx, val, err + (ulp(val, out_dt) if out_dt != torch.float32 else 0), "out")
    if out2:
        idx = store_index(M, N, ldo + 8, out_map=out_map, pixel_shuffle=pixel_shuffle)
        dt2 = out2_s.buf.dtype
        out2_s.check(idx, val, err + (ulp(val, dt2) if dt2 != torch.float32 else 0), "out2")
    if records:
        nrec = M * (N // 32) * 64
        r4 = rec[:nrec].view(M, N // 32, 2, 32).double()
        hi, lo = r4[:, :, 0].reshape(M, N), r4[:, :, 1].reshape(M, N)
        assert not (torch.isnan(hi).any() or torch.isnan(lo).any()), "records: elements left unwritten"
        bad = ~((hi + lo - val).abs() <= err + 2.0 ** -17 * val.abs())
        assert not bad.any(), f"records: {int(bad.sum())} elements of hi + lo off the reference"
        assert (rec[nrec:].view(torch.uint8) == 0).all(), "records: the 256-byte zero page is not zero"
    if splitk:
        assert (kw["splitk_scratch"] == 0).all(), "split-K scratch not left zeroed"
    return path


gpu = pytest.mark.gpu

# ---------------------------------------------------------------------------------------------------------------------
# generic kernel: three tiles x (prec, A dtype) x feature sets
# ---------------------------------------------------------------------------------------------------------------------
GEN_TILES = {"64x64": (300, 100, 96), "128x64": (16400, 60, 64), "128x128": (2000, 1040, 64)}
GEN_PRECS = {"x3_a32": (PREC_BF16X3, torch.float32, torch.float32), "x3_a16": (PREC_BF16X3, torch.bfloat16, torch.float32),
             "bf16_a32": (PREC_BF16, torch.float32, torch.bfloat16), "bf16_a16": (PREC_BF16, torch.bfloat16, torch.bfloat16),
             "f16_a32": (PREC_F16, torch.float32, torch.float16), "f16_a16": (PREC_F16, torch.float16, torch.float16)}


def _features(name, prec, N):
    """descriptor features of one generic-kernel cell (the mode's 16-bit format where a 16-bit type appears)"""
    h = H16[prec]
    return {
        "gelu_bias": dict(act=ACT_GELU, bias=True),
        "silu_gamma_resid_map_out2": dict(act=ACT_SILU, bias=True, gamma=True, resid=torch.float32,
                                          resid_map=(37, 45, 3), out2=True),
        "sigmoid_resid16_bcast_out16_out2": dict(act=ACT_SIGMOID, resid=h, resid_map=(50, 0, 1), out_dt=h, out2=True),
        "relu_resid_resid2_postgelu_outmap": dict(act=ACT_RELU, bias=True, resid=torch.float32, resid2=True,
                                                  post_act=ACT_GELU, out_map=(41, 47, 5)),
        "gamma_resid2_postsigmoid_misaligned": dict(gamma=True, resid2=True, post_act=ACT_SIGMOID, out_off=1),
        "gelu_out16_ldo_odd": dict(act=ACT_GELU, bias=True, out_dt=h, ldo_pad=3),
        "silu_n_ragged": dict(act=ACT_SILU, bias=True, resid=torch.float32, N=N - 1),
        "resid16_resid2_postrelu_outmap_out2": dict(resid=h, resid_map=(0, 0, 2), resid2=True, post_act=ACT_RELU,
                                                    out_map=(0, 0, 3), out2=True, out_dt=h),
    }[name]


GEN_FEATS = ["gelu_bias", "silu_gamma_resid_map_out2", "sigmoid_resid16_bcast_out16_out2",
             "relu_resid_resid2_postgelu_outmap", "gamma_resid2_postsigmoid_misaligned", "gelu_out16_ldo_odd",
             "silu_n_ragged", "resid16_resid2_postrelu_outmap_out2"]


def _gen_case(tile, pk, feat):
    M, N, K = GEN_TILES[tile]
    prec, a_dt, w_dt = GEN_PRECS[pk]
    f = dict(_features(feat, prec, N))
    N = f.pop("N", N)
    if f.get("out_dt") == torch.float16 and prec != PREC_F16:
        f["out_dt"] = torch.bfloat16
    return dict(M=M, N=N, K=K, prec=prec, a_dt=a_dt, w_dt=w_dt, **f)


@gpu
@pytest.mark.parametrize("feat", GEN_FEATS)
@pytest.mark.parametrize("pk", list(GEN_PRECS))
@pytest.mark.parametrize("tile", list(GEN_TILES))
def test_generic(tile, pk, feat, monkeypatch):
    c = _gen_case(tile, pk, feat)
    run_case(monkeypatch, **c, seed=100 * list(GEN_TILES).index(tile) + 10 * list(GEN_PRECS).index(pk) + GEN_FEATS.index(feat),
             expect=dict(family="generic", tile=tile, splitk=1))


@gpu
@pytest.mark.parametrize("act", [ACT_SIGMOID, ACT_SILU, ACT_GELU])
def test_generic_n1(act, monkeypatch):
    """N = 1 (the track head's visibility / confidence: sigmoid(Linear(128 -> 1)))"""
    run_case(monkeypatch, M=777, N=1, K=128, act=act, bias=True, expect=dict(family="generic", tile="64x64"))


@gpu
def test_generic_pixel_shuffle(monkeypatch):
    """store_mode 1 (ConvTranspose2d with kernel == stride) with bias, out2 and a residual"""
    cN, cH, cW, s, cout = 2, 9, 11, 2, 36
    run_case(monkeypatch, M=cN * cH * cW, N=s * s * cout, K=64, bias=True, act=ACT_RELU, out2=True, ldo_pad=4,
             pixel_shuffle=(s, cout, cN, cH, cW), expect=dict(family="generic"))


@gpu
@pytest.mark.parametrize("pk", list(GEN_PRECS))
def test_generic_random_data(pk, monkeypatch):
    prec, a_dt, w_dt = GEN_PRECS[pk]
    run_case(monkeypatch, M=300, N=100, K=512, prec=prec, a_dt=a_dt, w_dt=w_dt, data="random", bias=True, act=ACT_GELU,
             expect=dict(family="generic", tile="64x64"))


# ---------------------------------------------------------------------------------------------------------------------
# split-K (second pass gemm_splitk_epilogue): ordered (one plane per split) and atomic (a one-plane scratch)
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("feat", GEN_FEATS)
@pytest.mark.parametrize("mode", ["ordered", "atomic"])
def test_splitk(mode, feat, monkeypatch):
    pk = "x3_a32" if GEN_FEATS.index(feat) % 2 == 0 else "bf16_a16"
    c = _gen_case("64x64", pk, feat)
    c["K"] = 384
    planes = 3 if mode == "ordered" else 1
    run_case(monkeypatch, **c, splitk=3, splitk_planes=planes, seed=GEN_FEATS.index(feat),
             expect=dict(family="splitk_" + mode, tile="64x64", splitk=3))


@gpu
@pytest.mark.parametrize("mode", ["ordered", "atomic"])
def test_splitk_second_launch_on_zeroed_scratch(mode, monkeypatch):
    """the split-K epilogue leaves the scratch zeroed: a second launch that says so (no memset) is exact too"""
    _env(monkeypatch, {})
    g = _gen(9)
    M, N, K = 200, 72, 384
    a64, w64 = _ints((M, K), 3, g), _ints((N, K), 7, g) * 2.0 ** -_k_shift(K)
    b = torch.randn(N, generator=g).to(DEV)
    a, w = a64.float().to(DEV), w64.float().to(DEV)
    planes = 3 if mode == "ordered" else 1
    sc = torch.full((planes * M * N,), float("nan"), device=DEV)
    want = (a64 @ w64.T + b.double().cpu())
    for zeroed in (False, True):
        out = ops.gemm(a, w, bias=b, splitk_scratch=sc, force_splitk=3, splitk_zeroed=zeroed)
        p = ops.gemm_last_path()
        assert p.family == "splitk_" + mode and p.splitk == 3, p
        torch.cuda.synchronize()
        assert ((out.double().cpu() - want).abs() <= 2 * U * want.abs()).all()
        assert (sc == 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# gemm256: EPI 0..3 x the four main loops x bf16 / fp16 x MFMA 16 / 32, ragged M and N
# ---------------------------------------------------------------------------------------------------------------------
LOOP_ENV = {"two_phase_256": {"SKIMI_GEMM256_MT3": 0, "SKIMI_GEMM256_W4": 0, "SKIMI_GEMM256_PP": 0},
            "two_phase_192": {"SKIMI_GEMM256_MT3": 1},
            "ping_pong": {"SKIMI_GEMM256_MT3": 0, "SKIMI_GEMM256_W4": 0, "SKIMI_GEMM256_PP": 1},
            "single_stream": {"SKIMI_GEMM256_MT3": 0, "SKIMI_GEMM256_W4": 1}}
G256_LOOPS = [(lp, mf) for lp in LOOP_ENV for mf in ((16, 32) if lp in ("ping_pong", "single_stream") else (32,))]
# EPI 0: the shared epilogue, reached by each of the features no compile-time epilogue has (rotated over the cells)
EPI0_VIA = [dict(out_map=(0, 0, 2)), dict(resid=torch.float32, resid2=True), dict(out2=True),
            dict(act=ACT_RELU, post_act=ACT_SIGMOID), dict(resid="h16", gamma=True)]


def _g256_cases():
    cases = []
    for dt in ("bf16", "f16"):
        for lp, mf in G256_LOOPS:
            if dt == "f16" and lp == "two_phase_256":
                continue   # the fp16 build runs the ping-pong loop in its place
            for epi in range(4):
                cases.append((dt, lp, mf, epi))
    return cases


@gpu
@pytest.mark.parametrize("dt,loop,mfma,epi", _g256_cases())
def test_gemm256(dt, loop, mfma, epi, monkeypatch):
    prec, h = (PREC_BF16, torch.bfloat16) if dt == "bf16" else (PREC_F16, torch.float16)
    i = _g256_cases().index((dt, loop, mfma, epi))
    with_bias = (i // 4) % 2 == 0   # bias absent / present on alternate loops, for every EPI
    c = dict(M=2300, N=520, K=128, prec=prec, a_dt=h, w_dt=h, bias=with_bias)
    if epi == 0:
        f = dict(EPI0_VIA[i % len(EPI0_VIA)])
        if f.get("resid") == "h16":
            f["resid"] = h
        c.update(f)
    elif epi == 1:
        c.update(out_dt=torch.bfloat16)
    elif epi == 3:
        c.update(act=ACT_GELU, out_dt=h)
    else:
        c.update(gamma=True, resid=torch.float32, inplace=i % 3 == 0)
    env = dict(LOOP_ENV[loop], SKIMI_GEMM256_MFMA=mfma)
    run_case(monkeypatch, **c, env=env, seed=i, expect=dict(family="gemm256", loop=loop, mfma=mfma, epi=epi))


@gpu
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_gemm256_random_data(dt, monkeypatch):
    prec, h = (PREC_BF16, torch.bfloat16) if dt == "bf16" else (PREC_F16, torch.float16)
    run_case(monkeypatch, M=2300, N=520, K=1024, prec=prec, a_dt=h, w_dt=h, data="random", bias=True, gamma=True,
             resid=torch.float32, expect=dict(family="gemm256", epi=2))


# ---------------------------------------------------------------------------------------------------------------------
# x3dma (LDS-DMA bf16x3, SKIMI_X3_MIN_TILES=1): the fast epilogue's nine variants (resid / resid2) x (out / records /
# both) on interior and ragged tiles, wide (N > 128) and narrow, plain rows, conv gather and A records; and the shared
# epilogue that serves everything the fast path does not
# ---------------------------------------------------------------------------------------------------------------------
X3_VARIANTS = [(res, o, rc) for res in (0, 1, 2) for (o, rc) in ((True, True), (True, False), (False, True))]
X3_SHAPES = {"wide": dict(M=612, N=352), "narrow": dict(M=612, N=128)}


def _x3_features(res, o, rc, i):
    f = dict(bias=i % 2 == 0, act=ACT_RELU if i % 3 != 1 else ACT_NONE, post_act=ACT_RELU if i % 2 else ACT_NONE,
             records=rc, out_dt=torch.float32 if o else None)
    if res >= 1:
        f.update(resid=torch.float32, resid_map=[(0, 0, 0), (100, 130, 7), (0, 0, 4)][i % 3])
    if res == 2:
        f.update(resid2=True)
    return f


# plain fp32 rows and A records: all nine variants; the conv gather: every third
X3_FAST = [(v, k, f) for f in ("rows", "records", "conv") for k in X3_SHAPES for v in range(len(X3_VARIANTS))
           if f != "conv" or v % 3 == 0]


@gpu
@pytest.mark.parametrize("variant,kind,a_form", X3_FAST)
def test_x3dma_fast(variant, kind, a_form, monkeypatch):
    res, o, rc = X3_VARIANTS[variant]
    c = dict(X3_SHAPES[kind], **_x3_features(res, o, rc, variant))
    if a_form == "conv":
        c.pop("M")
        c["conv"] = dict(N=2, H=18, W=17, C=32, KH=3, KW=3, stride=1, pad=1)
    else:
        c["K"] = 160
    run_case(monkeypatch, **c, w_split=True, a_records=a_form == "records", env={"SKIMI_X3_MIN_TILES": 1}, seed=variant,
             expect=dict(family="x3dma_" + kind, splitk=1))


X3_FALLBACK = {"gamma": dict(gamma=True, bias=True, resid=torch.float32), "gelu": dict(act=ACT_GELU, bias=True),
               "out_map": dict(out_map=(300, 310, 2), resid=torch.float32, resid2=True),
               "resid16": dict(resid=torch.bfloat16, resid_map=(0, 0, 1), act=ACT_RELU),
               "silu_out2": dict(act=ACT_SILU, out2=True), "post_sigmoid": dict(post_act=ACT_SIGMOID, resid2=True)}


@gpu
@pytest.mark.parametrize("feat", list(X3_FALLBACK))
@pytest.mark.parametrize("kind", list(X3_SHAPES))
def test_x3dma_shared_epilogue(kind, feat, monkeypatch):
    run_case(monkeypatch, **X3_SHAPES[kind], K=96, **X3_FALLBACK[feat], w_split=True, env={"SKIMI_X3_MIN_TILES": 1},
             expect=dict(family="x3dma_" + kind))


@gpu
@pytest.mark.parametrize("kind", list(X3_SHAPES))
def test_x3dma_random_data(kind, monkeypatch):
    run_case(monkeypatch, **X3_SHAPES[kind], K=800, data="random", bias=True, resid=torch.float32, w_split=True,
             env={"SKIMI_X3_MIN_TILES": 1}, expect=dict(family="x3dma_" + kind))


# ---------------------------------------------------------------------------------------------------------------------
# conv_win (3x3 / 128 channels on 16-bit operands, SKIMI_CONV_WIN=2)
# ---------------------------------------------------------------------------------------------------------------------
CW_FEATS = {"bias_relu": dict(bias=True, act=ACT_RELU),
            "resid_resid2_post": dict(resid="h16", resid2=True, post_act=ACT_RELU, bias=True),
            "out2": dict(bias=True, act=ACT_GELU, out2=True),
            "out16": dict(out_dt="h16", act=ACT_SILU, gamma=True),
            "out16_out2_resid32": dict(out_dt="h16", out2=True, resid=torch.float32, resid_map=(0, 0, 3))}


@gpu
@pytest.mark.parametrize("feat", list(CW_FEATS))
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_conv_win(dt, feat, monkeypatch):
    prec, h = (PREC_BF16, torch.bfloat16) if dt == "bf16" else (PREC_F16, torch.float16)
    f = {k: (h if v == "h16" else v) for k, v in CW_FEATS[feat].items()}
    run_case(monkeypatch, N=128, prec=prec, a_dt=h, w_dt=h, conv=dict(N=2, H=20, W=23, C=64, KH=3, KW=3, stride=1, pad=1),
             **f, env={"SKIMI_CONV_WIN": 2}, expect=dict(family="conv_win", splitk=1))


@gpu
def test_conv_win_random_data(monkeypatch):
    run_case(monkeypatch, N=128, prec=PREC_BF16, a_dt=torch.bfloat16, w_dt=torch.bfloat16, data="random", bias=True,
             conv=dict(N=2, H=20, W=23, C=64, KH=3, KW=3, stride=1, pad=1), env={"SKIMI_CONV_WIN": 2},
             expect=dict(family="conv_win"))


# ---------------------------------------------------------------------------------------------------------------------
# forward replays: the descriptor each forward call site builds, at its real shape
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_replay_patch_embed(dt, monkeypatch):
    """vggt.hip (forward_impl) patch embed at VGGT-1B size, 8 frames of 518^2: patches of each frame land behind its 5 special
    tokens (out_row_off 5, frame stride P = 1374), + the DINO pos_embed broadcast over frames (batch stride 0,
    row offset 1).  K = 3*14*14 padded to 592 (not a multiple of 64): the generic 128x128 kernel, not gemm256."""
    prec, h = (PREC_BF16, torch.bfloat16) if dt == "bf16" else (PREC_F16, torch.float16)
    F_, np_, nsp, C = 8, 37 * 37, 5, 1024
    run_case(monkeypatch, M=F_ * np_, N=C, K=592, prec=prec, a_dt=h, w_dt=h, bias=True, resid=torch.float32,
             resid_map=(np_, 0, 1), resid_rows=1 + np_, out_map=(np_, np_ + nsp, nsp),
             expect=dict(family="generic", tile="128x128", splitk=1))


@gpu
@pytest.mark.parametrize("mode", ["x3_records", "bf16"])
def test_replay_dpt_rcu1(mode, monkeypatch):
    """vggt_dpt.hip DPT fusion RCU1 conv2: 3x3 conv feat -> feat, + relu(x) (resid, the mode's activation dtype)
    + prev (resid2) then ReLU; fp32-accurate mode with its records output on the LDS-DMA kernel"""
    conv = dict(N=8, H=74, W=74, C=256, KH=3, KW=3, stride=1, pad=1)   # 43808 rows: 172 tiles of 256
    if mode == "x3_records":
        run_case(monkeypatch, N=256, conv=conv, bias=True, resid=torch.float32, resid2=True, post_act=ACT_RELU,
                 records=True, w_split=True, expect=dict(family="x3dma_wide"))
    else:
        run_case(monkeypatch, N=256, conv=conv, prec=PREC_BF16, a_dt=torch.bfloat16, w_dt=torch.bfloat16, bias=True,
                 resid=torch.bfloat16, resid2=True, post_act=ACT_RELU, out_dt=torch.bfloat16,
                 expect=dict(family="generic", tile="128x128"))


@gpu
@pytest.mark.parametrize("route", ["generic", "x3dma"])
def test_replay_vp3d_block(route, monkeypatch):
    """vp3d.hip block: conv 1x1 + BN + ReLU, + x[:, pad + shift : L - pad + shift] (residual rows per clip with the
    clip stride L and offset pad + shift), 1024 channels, 64 clips of a 3-dilated block (L = 81 -> 75)"""
    env = {"SKIMI_X3_MIN_TILES": 1} if route == "x3dma" else {}
    run_case(monkeypatch, M=64 * 75, N=1024, K=1024, bias=True, act=ACT_RELU, resid=torch.float32,
             resid_map=(75, 81, 3), w_split=True, env=env,
             expect=dict(family="generic" if route == "generic" else "x3dma_wide"))


@gpu
def test_replay_track_fc2(monkeypatch):
    """vggt_track.hip transformer fc2: + x (resid) + the other stream's tokens (resid2), hidden 384"""
    run_case(monkeypatch, M=8 * 256, N=384, K=4 * 384, bias=True, resid=torch.float32, resid2=True,
             expect=dict(family="generic"))


@gpu
def test_replay_track_vis_conf(monkeypatch):
    """vggt_track.hip visibility / confidence: sigmoid(Linear(128 -> 1)) over B*N*S rows"""
    run_case(monkeypatch, M=2 * 256 * 8, N=1, K=128, bias=True, act=ACT_SIGMOID, expect=dict(family="generic"))


@gpu
def test_replay_camera_embed_pose(monkeypatch):
    """vggt_camera.hip camera head: poseLN_modulation embed, SiLU(Linear(16 -> 2048)) of 8 frames' pose codes"""
    run_case(monkeypatch, M=8, N=2048, K=16, bias=True, act=ACT_SILU, expect=dict(family="generic", tile="64x64"))
