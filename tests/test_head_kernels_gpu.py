"""GPU: every VGGT head / track-head helper kernel on its own (include/skimi.h, "VGGT head and track-head helper
kernels") against the float64 restatements of head_kernels_restated.py, at tiny shapes.

Every output is prefilled with 0xFF bytes (NaN in fp32, bf16 and fp16) and sits between two 256-byte guards that must
come back untouched.  Every tolerance is a forward error bound computed from the reference's own magnitudes in units of
u = 2^-24 (never from the kernel's output); the worst error / bound per kernel is recorded (profiles/head_kernels_unit.md;
SKIMI_HEAD_KERNEL_RATIOS=<file> writes them as JSON).  Pure data movement is compared bit for bit."""
import json
import math
import os

import numpy as np
import pytest
import torch

import head_kernels_restated as R
from skiing_analysis_pytorch_amd import _lib, ops

pytestmark = pytest.mark.gpu

U = R.U
GUARD = 256
FLT_MAX = 3.4028234663852886e38
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
RATIOS = {}


@pytest.fixture(scope="module", autouse=True)
def _report_ratios():
    yield
    for k in sorted(RATIOS):
        print(f"worst error / bound  {k:40s} {RATIOS[k]:.3f}")
    path = os.environ.get("SKIMI_HEAD_KERNEL_RATIOS")
    if path:
        with open(path, "w") as f:
            json.dump(RATIOS, f, indent=1, sort_keys=True)


class Guarded:
    """a device buffer of `shape` x `dtype`, all 0xFF, with GUARD bytes of 0xFF in front of and behind it"""

    def __init__(self, dtype, shape):
        self.nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        self.full = torch.full((GUARD + self.nbytes + GUARD,), 0xFF, dtype=torch.uint8, device="cuda")
        self.t = self.full[GUARD:GUARD + self.nbytes].view(dtype).view(*shape)

    def check(self):
        c = self.full.cpu().numpy()
        assert (c[:GUARD] == 0xFF).all(), "bytes in front of the output were written"
        assert (c[GUARD + self.nbytes:] == 0xFF).all(), "bytes behind the output were written"


def _rng(seed):
    return np.random.default_rng(seed)


def _dev(a, dt=torch.float32):
    """float array -> (device tensor of type dt, the float64 values it holds)"""
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dt)
    return t.cuda(), t.double().numpy()


def _np(t):
    return t.detach().cpu().double().numpy()


def _bits16(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def _check(key, got, ref, tol):
    """|got - ref| <= tol everywhere (a NaN fails; where the reference overflows fp32 the kernel must give that inf);
    records the worst error / bound under `key`"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    tol = np.broadcast_to(np.asarray(tol, np.float64), ref.shape)
    over = np.abs(ref) > FLT_MAX
    assert np.array_equal(got[over], np.sign(ref[over]) * np.inf), f"{key}: overflow must give inf"
    err, t = np.abs(got[~over] - ref[~over]), tol[~over]
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(t > 0, err / t, np.where(err == 0, 0.0, np.inf))
    worst = float(ratio.max()) if ratio.size else 0.0
    worst = math.inf if math.isnan(worst) else worst
    RATIOS[key] = max(RATIOS.get(key, 0.0), worst)
    print(f"{key}: worst error / bound {worst:.3f}, max abs error {np.nanmax(err) if err.size else 0.0:.3e}")
    bad = np.argwhere(~over)[~(ratio <= 1.0)] if worst > 1.0 else []
    assert worst <= 1.0, f"{key}: error / bound = {worst}; {len(bad)} elements over the bound, the first at {list(bad[:4])}"


def _tables(H, W, C, seed):
    g = _rng(seed)
    tx, ty = g.standard_normal((W, C // 2)).astype(np.float32) * 0.1, g.standard_normal((H, C // 2)).astype(np.float32) * 0.1
    return torch.from_numpy(tx).cuda(), torch.from_numpy(ty).cuda(), tx.astype(np.float64), ty.astype(np.float64)


# ------------------------------------------------------------------------------------------------------------------
# resize
# ------------------------------------------------------------------------------------------------------------------
RESIZE_SHAPES = [((3, 5), (7, 12)), ((4, 4), (4, 4)), ((9, 9), (4, 5)), ((1, 6), (5, 6)), ((6, 1), (6, 3)), ((5, 7), (1, 1)),
                 ((10, 10), (37, 37)), ((37, 37), (74, 74))]
TYPE_PAIRS = [("f32", "f32"), ("bf16", "bf16"), ("f16", "f16"), ("bf16", "f32"), ("f16", "f32")]


@pytest.mark.parametrize("C", [4, 8, 36, 128])
@pytest.mark.parametrize("src,dst", RESIZE_SHAPES)
def test_resize(src, dst, C):
    """fp32 out: 8u on the absolute-value lerp (+ |uv|): seven roundings and the table add.  16-bit out: plus half a
    unit in the last place of the output format at the reference value.  16-bit in: the reference starts from the
    decoded inputs.  The identity is bit exact in fp32."""
    N, (h, w), (H, W) = 2, src, dst
    x32 = _rng(100 + C).standard_normal((N, h, w, C)) * 2.0
    tx, ty, txn, tyn = _tables(H, W, C, 7) if C % 8 == 0 else (None,) * 4
    refs = {}
    for tin, tout in TYPE_PAIRS:
        x, xv = _dev(x32, DT[tin])
        for tab in ([False, True] if C % 8 == 0 else [False]):
            if (tin, tab) not in refs:
                refs[tin, tab] = R.resize(xv, H, W, txn if tab else None, tyn if tab else None)
            ref, mag = refs[tin, tab]
            out = Guarded(DT[tout], (N, H, W, C))
            ops.resize_bilinear(x, H, W, out=out.t, tabx=tx if tab else None, taby=ty if tab else None)
            out.check()
            tol = 8 * U * mag + (R.half_ulp16(ref, tout == "f16") if tout != "f32" else 0.0)
            _check(f"resize {tin}->{tout}" + (" +uv" if tab else ""), _np(out.t), ref, tol)
            if src == dst and tin == "f32" and not tab:
                assert torch.equal(out.t, x), "the identity resize must be bit exact"


LN_SHAPES = {3: ((3, 2), (5, 3)), 12: ((3, 5), (7, 12)), 74: ((37, 37), (74, 74))}


@pytest.mark.parametrize("case", ["random", "constant_per_pixel", "mean_1e3"])
@pytest.mark.parametrize("W", [3, 12, 74])
def test_resize_layernorm(W, case):
    """resize + LayerNorm (C = 128, fp32 out).  With eps the largest lerp bound 8u mag of the pixel's channels, the
    centred value is off by at most 2 eps (its own error and the mean's) and by the 4u max|r - mean| of the fp32 mean
    and subtraction; the scale by rstd and gamma and the beta add are 4u |out|."""
    N, C, ln_eps = 2, 128, 1e-5
    (h, w), (H, _) = LN_SHAPES[W]
    g = _rng(200 + W)
    if case == "random":
        x32 = g.standard_normal((N, h, w, C)) * 2.0
    elif case == "constant_per_pixel":
        x32 = np.repeat(g.standard_normal((N, h, w, 1)) * 3.0, C, axis=3)
    else:
        x32 = 1e3 + g.standard_normal((N, h, w, C))
    gam, gamn = _dev(g.standard_normal(C))
    bet, betn = _dev(g.standard_normal(C))
    for tin in ("f32", "bf16", "f16"):
        x, xv = _dev(x32, DT[tin])
        v, mag = R.resize(xv, H, W)
        ref, cen, rstd = R.layernorm(v, gamn, betn, ln_eps)
        eps = (8 * U * mag).max(axis=-1, keepdims=True)
        tol = (2 * eps + 4 * U * np.abs(cen).max(axis=-1, keepdims=True)) * rstd * np.abs(gamn) + 4 * U * np.abs(ref)
        out = Guarded(torch.float32, (N, H, W, C))
        ops.resize_bilinear(x, H, W, out=out.t, ln_g=gam, ln_b=bet, ln_eps=ln_eps)
        out.check()
        _check(f"resize+LN {tin} {case}", _np(out.t), ref, tol)
        if case == "constant_per_pixel":   # variance exactly 0: (r - mean) = 0 in the kernel too
            assert np.array_equal(_np(out.t), np.broadcast_to(betn, (N, H, W, C))), "zero variance must give beta"


def _check_hi_lo(key, rec, slot, lo_off, ref, tol_fp32):
    """rec [pixels, 2C] bf16 patterns: hi + lo against ref within the fp32 bound + 2^-16 |v| (lo's own rounding: half an
    ulp of a value that is at most half an ulp of hi); and hi is the bf16 NEAREST to the decoded sum -- what
    hi == RNE-bf16(v) implies for v = hi + lo up to lo's rounding (at an exact tie of the decoded sum the v the kernel
    held is on either side, so even / odd is not asserted there)"""
    hb, lb = rec[:, slot], rec[:, slot + lo_off]
    hi, lo = R.decode16(hb, False), R.decode16(lb, False)
    _check(key, (hi + lo).reshape(ref.shape), ref, tol_fp32 + 2.0 ** -16 * np.abs(ref))
    nz = (hb & 0x7FFF) != 0
    up, dn = R.decode16(hb + np.uint16(1), False), R.decode16(hb - np.uint16(1), False)
    s = hi + lo
    assert (np.abs(lo)[nz] <= np.abs(s - up)[nz]).all() and (np.abs(lo)[nz] <= np.abs(s - dn)[nz]).all(), \
        f"{key}: hi is not the bf16 nearest to hi + lo"
    assert (lo[~nz] == 0).all()


@pytest.mark.parametrize("tab", [False, True])
@pytest.mark.parametrize("C,records", [(16, False), (32, False), (64, False), (32, True), (64, True)])   # records: C % 32 == 0
def test_resize_planes(C, records, tab):
    N = 2
    slot, lo_off = R.plane_slots(C, records)
    for (h, w), (H, W) in (((3, 5), (7, 12)), ((10, 10), (37, 37))):
        x32 = _rng(300 + C).standard_normal((N, h, w, C)) + 0.37 * np.arange(1, C + 1)     # every channel differs
        x, xv = _dev(x32)
        tx, ty, txn, tyn = _tables(H, W, C, 8) if tab else (None,) * 4
        ref, mag = R.resize(xv, H, W, txn, tyn)
        out = Guarded(torch.int16, (N * H * W * 2 * C + 128,))      # records, then the 256-byte zero page
        zpage = out.t[N * H * W * 2 * C:]
        ops.resize_bilinear_planes(x, H, W, out.t, tabx=tx, taby=ty, records=records, zpage=zpage)
        out.check()
        bits = _bits16(out.t)
        assert not bits[N * H * W * 2 * C:].any(), "the zero page must read back as 256 zero bytes"
        _check_hi_lo(f"resize planes {'records' if records else 'planes'}" + (" +uv" if tab else ""),
                     bits[:N * H * W * 2 * C].reshape(N * H * W, 2 * C), slot, lo_off, ref.reshape(N * H * W, C),
                     8 * U * mag.reshape(N * H * W, C))


# ------------------------------------------------------------------------------------------------------------------
# UV add
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("C", [8, 24, 128])
def test_add_uv_pos(C, dt):
    """one fp32 add, then one rounding to the map's type: bit for bit"""
    N, H, W = 2, 3, 5
    x, xv = _dev(_rng(400 + C).standard_normal((N, H, W, C)), DT[dt])
    tx, ty, txn, tyn = _tables(H, W, C, 9)
    buf = Guarded(DT[dt], (N, H, W, C))
    buf.t.copy_(x)
    ops.add_uv_pos_(buf.t, tx, ty)
    buf.check()
    want = (x.cpu().float() + torch.from_numpy(R.uv_add(H, W, txn, tyn).astype(np.float32))[None]).to(DT[dt])
    assert torch.equal(buf.t.cpu(), want)


@pytest.mark.parametrize("tab", [False, True])
@pytest.mark.parametrize("C", [32, 96])
def test_add_uv_pos_records(C, tab):
    N, H, W = 2, 3, 5
    npix = N * H * W
    x, xv = _dev(_rng(500 + C).standard_normal((N, H, W, C)) + 0.37 * np.arange(1, C + 1))
    keep = x.clone()
    tx, ty, txn, tyn = _tables(H, W, C, 10) if tab else (None,) * 4
    ref = xv + (R.uv_add(H, W, txn, tyn)[None] if tab else 0.0)
    rec = Guarded(torch.int16, (npix * 2 * C + 128,))
    ops.add_uv_pos_records(x, rec.t, tx, ty)
    rec.check()
    assert torch.equal(x, keep), "x must be left as it is"
    bits = _bits16(rec.t)
    assert not bits[npix * 2 * C:].any(), "the zero page must read back as 256 zero bytes"
    slot, lo_off = R.plane_slots(C, True)
    _check_hi_lo("uv add records" + (" +uv" if tab else ""), bits[:npix * 2 * C].reshape(npix, 2 * C), slot, lo_off,
                 ref.reshape(npix, C), (U * np.abs(ref) if tab else np.zeros_like(ref)).reshape(npix, C))


# ------------------------------------------------------------------------------------------------------------------
# DPT output stage
# ------------------------------------------------------------------------------------------------------------------
def _dpt_check(key, pts, conf, y, mag, mode, rel_pts=None):
    """|dy| <= 34u (sum |v w| + |b|); exp needs relative |dy| + 4u (expf / expm1f), sign(y) expm1(|y|) the derivative
    exp(|y|) |dy| + 4u |pts|, conf one more rounding; fp32 results below the normal range may be flushed (2^-126)"""
    dy = 34 * U * mag
    rp, rc = R.dpt_act(y, mode)
    with np.errstate(over="ignore", invalid="ignore"):
        if rel_pts is not None:
            tp = rel_pts * np.abs(rp)
        elif mode == 0:
            tp = (np.expm1(dy[:, :-1]) + 4 * U) * np.abs(rp) + R.F32_TINY
        else:
            tp = np.exp(np.abs(y[:, :-1]) + dy[:, :-1]) * dy[:, :-1] + 4 * U * np.abs(rp) + R.F32_TINY
        tc = (np.expm1(dy[:, -1]) + 4 * U) * np.exp(y[:, -1]) + U * np.abs(rc) + R.F32_TINY
    _check(key + " pts", pts, rp, tp)
    _check(key + " conf", conf, rc, tc)


@pytest.mark.parametrize("n_out", [2, 4])
@pytest.mark.parametrize("npix", [1, 255, 256, 257, 5000])
def test_dpt_out(npix, n_out):
    g = _rng(600 + npix)
    x32 = np.abs(g.standard_normal((npix, 32)))
    w, wn = _dev(g.standard_normal((n_out, 32)) * 0.3)
    b, bn = _dev(g.standard_normal(n_out))
    for dt in ("f32", "bf16", "f16"):
        x, xv = _dev(x32, DT[dt])
        y, mag = R.dpt_pre(xv, wn, bn)
        for mode in (0, 1):
            pts, conf = Guarded(torch.float32, (npix, n_out - 1)), Guarded(torch.float32, (npix,))
            ops.dpt_out(x, w, b, mode, pts=pts.t, conf=conf.t)
            pts.check(), conf.check()
            _dpt_check(f"dpt_out {dt} {'exp' if mode == 0 else 'inv_log'}", _np(pts.t), _np(conf.t), y, mag, mode)


@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("n_out", [2, 4])
def test_dpt_out_chosen_values(n_out, dt):
    """one-hot weights: the pre-activation is input channel 0 itself, exactly"""
    vals = np.array([0.0, 1e-6, -1e-6, 20.0, -20.0, 100.0, -100.0, 0.5])
    npix = len(vals)
    x32 = np.abs(_rng(700).standard_normal((npix, 32)))
    x32[:, 0] = vals
    x, xv = _dev(x32, DT[dt])
    wn = np.zeros((n_out, 32))
    wn[:, 0] = 1.0
    w, _ = _dev(wn)
    b, bn = _dev(np.zeros(n_out))
    y, mag = R.dpt_pre(xv, wn, bn)
    assert np.array_equal(y[:, 0], xv[:, 0])
    for mode in (0, 1):
        pts, conf = Guarded(torch.float32, (npix, n_out - 1)), Guarded(torch.float32, (npix,))
        ops.dpt_out(x, w, b, mode, pts=pts.t, conf=conf.t)
        pts.check(), conf.check()
        p, c = _np(pts.t), _np(conf.t)
        _dpt_check(f"dpt_out chosen {dt} {'exp' if mode == 0 else 'inv_log'}", p, c, y, mag, mode)
        assert c[0] == 2.0 and c[5] == np.inf
        if mode == 1:
            assert (p[0] == 0.0).all() and (p[5] == np.inf).all() and (p[6] == -np.inf).all()
            # y = +-1e-6 (as the input type holds it): relative 8u, which exp(y) - 1 misses by orders of magnitude
            _dpt_check(f"dpt_out 1e-6 {dt}", p[1:3], c[1:3], y[1:3], mag[1:3], 1, rel_pts=8 * U)
        else:
            assert (p[0] == 1.0).all() and (p[5] == np.inf).all()


# ------------------------------------------------------------------------------------------------------------------
# patch gather, AdaLN, pose update, special tokens
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("H,W,p,Kp", [(28, 42, 14, 588), (28, 42, 14, 592), (8, 12, 4, 64)])
def test_patch_gather(H, W, p, Kp, dt):
    """(x - mean) / std: two fp32 roundings, 2u |v| (+ half an ulp of a 16-bit output); padding columns are zero bits"""
    img, imgv = _dev(_rng(800).uniform(0, 1, (2, 3, H, W)))
    ref, _ = R.patch_gather(imgv, p, Kp)
    out = Guarded(DT[dt], ref.shape)
    ops.patch_gather(img, p, Kp, out=out.t)
    out.check()
    tol = 2 * U * np.abs(ref) + (R.half_ulp16(ref, dt == "f16") if dt != "f32" else 0.0)
    tol[:, 3 * p * p:] = 0.0
    _check(f"patch_gather {dt}", _np(out.t), ref, tol)
    pad = out.t[:, 3 * p * p:].cpu().contiguous()
    if pad.numel():
        assert not pad.view(torch.int16 if dt != "f32" else torch.int32).any(), "padding columns must be exactly 0"


@pytest.mark.parametrize("rows,D", [(3, 8), (5, 2048)])
def test_adaln(rows, D):
    """gate * (xn * (1 + scale) + shift) + x: five fp32 roundings, 6u on the absolute-value evaluation"""
    g = _rng(900 + D)
    xn, xnv = _dev(g.standard_normal((rows, D)))
    x, xv = _dev(g.standard_normal((rows, D)))
    mod, modv = _dev(g.standard_normal((rows, 3 * D)))
    ref, mag = R.adaln(xnv, xv, modv)
    out = Guarded(torch.float32, (rows, D))
    ops.adaln(xn, x, mod, out=out.t)
    out.check()
    _check("adaln", _np(out.t), ref, 6 * U * mag)


def test_pose_update():
    """first = 1 copies, first = 0 is one fp32 add: bit for bit; columns 9..15 of pred_pad keep their bytes"""
    rows = 5
    g = _rng(1000)
    d1, d2 = g.standard_normal((rows, 9)).astype(np.float32), g.standard_normal((rows, 9)).astype(np.float32)
    pad = Guarded(torch.float32, (rows, 16))
    padn = pad.t.cpu().numpy().copy()      # all NaN patterns: a copy must not care what was there
    for delta, first in ((d1, 1), (d2, 0)):
        act = Guarded(torch.float32, (rows, 9))
        ops.pose_update_(torch.from_numpy(delta).cuda(), pad.t, act.t, first)
        pad.check(), act.check()
        padn, actn = R.pose_update(delta, padn, bool(first))
        assert np.array_equal(pad.t.cpu().numpy().view(np.uint32), padn.view(np.uint32))
        assert np.array_equal(act.t.cpu().numpy().view(np.uint32), actn.view(np.uint32))
    assert (pad.t.cpu().numpy().view(np.uint32)[:, 9:] == 0xFFFFFFFF).all()


def test_special_tokens():
    F, S, P, n, C = 4, 2, 7, 3, 8
    g = _rng(1100)
    x0 = g.standard_normal((F, P, C)).astype(np.float32)
    table = g.standard_normal((2, n, C)).astype(np.float32)
    x = Guarded(torch.float32, (F, P, C))
    x.t.copy_(torch.from_numpy(x0))
    ops.special_tokens_(x.t, torch.from_numpy(table).cuda(), S)
    x.check()
    got = x.t.cpu().numpy()
    assert np.array_equal(got, R.special_tokens(x0, table, S))
    assert np.array_equal(got[:, n:], x0[:, n:]), "rows n..P-1 must be untouched"


# ------------------------------------------------------------------------------------------------------------------
# track head
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [3, 64])
@pytest.mark.parametrize("H,W", [(6, 8), (7, 9)])
def test_track_avgpool2(H, W, C):
    """(a + b + c + d) * 0.25: three roundings, 4u on the mean of absolute values"""
    x, xv = _dev(_rng(1200 + C).standard_normal((2, H, W, C)))
    ref, mag = R.avgpool2(xv)
    out = Guarded(torch.float32, ref.shape)
    ops.track_avgpool2(x, out=out.t)
    out.check()
    _check("avgpool2", _np(out.t), ref, 4 * U * mag)


# (H, W) = (5, 9): interior fractional, exact integers, exactly (W-1, H-1), left of the map, right of and above it,
# just outside the corner, and two more fractional ones
HAND_COORDS = [(3.3, 1.7), (2.0, 3.0), (8.0, 4.0), (-3.5, 2.0), (19.0, -1.0), (-0.5, -0.25), (7.25, 0.5), (0.0, 3.999)]


def _dyadic(c):
    c = np.asarray(c, np.float32).astype(np.float64)
    return (c * 64 == np.round(c * 64)).all(axis=-1)


def _coords_buffer(coords, stride):
    """coords [R, 2] -> device [R, stride] with 1e3 in the slots nobody may read"""
    buf = np.full((coords.shape[0], stride), 1e3, np.float32)
    buf[:, :2] = coords
    return torch.from_numpy(buf).cuda()


@pytest.mark.parametrize("coord_stride", [2, 6])
@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("C", [3, 64])
def test_track_sample_border(C, padded, coord_stride):
    """6u sum w |v| (two weight roundings, two products, three adds at most per term); where a coordinate is not dyadic
    the weight 1 - l is rounded: u times the clamped coordinate times the local slope"""
    B, N, H, W = 2, 8, 5, 9
    g = _rng(1300 + C)
    img_stride = 2 * H * W * C if padded else H * W * C     # the forward passes S * H * W * C
    fm = g.standard_normal((B, img_stride)).astype(np.float32)
    coords = np.stack([np.array(HAND_COORDS, np.float32), np.array(HAND_COORDS[::-1], np.float32)])
    ref, mag, slope = R.sample_border(fm[:, :H * W * C].reshape(B, H, W, C), coords)
    out = Guarded(torch.float32, (B, N, C))
    ops.track_sample_border(torch.from_numpy(fm).cuda(), img_stride, _coords_buffer(coords.reshape(-1, 2), coord_stride),
                            coord_stride, B, N, H, W, C, out=out.t)
    out.check()
    tol = 6 * U * mag + U * slope * (~_dyadic(coords))[..., None]
    _check("sample_border", _np(out.t), ref, tol)


@pytest.mark.parametrize("C,r,level", [(16, 1, 0), (96, 3, 0), (64, 3, 2), (128, 1, 1)])
def test_track_corr_sample(C, r, level):
    """against the materialised correlation volume sampled by grid_sample (zeros padding).  Coordinates are dyadic, so
    every coordinate, floor and weight is exact in fp32 and only products and sums round: (C + 8) u on the same
    formula evaluated on |target| and |fmap|.  The float64 reference normalises the grid and grid_sample undoes it: a
    coordinate error below 1e-14, times the largest correlation magnitude of the row, is added for that."""
    B, N, S, H, W = 2, 3, 2, 12, 16
    rows, side = B * N * S, 2 * r + 1
    ns, g = side * side, _rng(1400 + C)
    tgt, tgtv = _dev(g.standard_normal((rows, C)))
    fmap, fmapv = _dev(g.standard_normal((B * S, H, W, C)))
    lvl = np.stack([g.integers(-2 * 64, (W + 1) * 64, rows, endpoint=True),
                    g.integers(-2 * 64, (H + 1) * 64, rows, endpoint=True)], axis=1) / 64.0
    lvl[1], lvl[5], lvl[9] = (-0.5, -0.25), (W - 1, H - 1), (W + 20, 0)
    coords = (lvl * 2 ** level).astype(np.float32)
    assert np.array_equal(coords.astype(np.float64), lvl * 2 ** level)
    ref, mag = R.corr_sample(tgtv, fmapv, coords, N, S, r, level)
    assert (ref != 0).mean() >= 1 / 3 and (ref == 0).mean() >= 1 / 10 and not ref[9].any()
    ldo, out_off = 3 * ns, ns
    out = Guarded(torch.float32, (rows, ldo))
    ops.track_corr_sample(tgt, fmap, torch.from_numpy(coords).cuda(), out.t, N, S, r, level, ldo, out_off)
    out.check()
    raw = out.t.cpu().numpy()
    assert (raw.view(np.uint32)[:, :out_off] == 0xFFFFFFFF).all() and (raw.view(np.uint32)[:, out_off + ns:] == 0xFFFFFFFF).all(), \
        "columns outside [out_off, out_off + (2r+1)^2) were written"
    slack = 1e-14 * (np.abs(tgtv).sum(axis=1) * np.abs(fmapv).max() / math.sqrt(C))[:, None]
    _check(f"corr_sample C={C} r={r} level={level}", raw[:, out_off:out_off + ns].astype(np.float64), ref,
           (C + 8) * U * mag + slack)


@pytest.mark.parametrize("coord_stride", [2, 6])
@pytest.mark.parametrize("D", [196, 388])
def test_track_pos_embed_sample(D, coord_stride):
    """table values rounded to fp32 on both sides, interpolated: 6u sum w |v| (+ the coordinate term off the dyadic grid)"""
    BN, H, W = 6, 5, 9
    coords = np.array(HAND_COORDS[:6], np.float32)
    ref, mag, slope = R.pos_embed_sample(coords, H, W, D)
    out = Guarded(torch.float32, (BN, D))
    ops.track_pos_embed_sample(_coords_buffer(coords, coord_stride), coord_stride, BN, H, W, D, out=out.t)
    out.check()
    _check("pos_embed_sample", _np(out.t), ref, 6 * U * mag + U * slope * (~_dyadic(coords))[:, None])


@pytest.mark.parametrize("L", [64, 128])
def test_track_input(L):
    """4u absolute on the sine / cosine columns (sinf / cosf of the fp32 angle) and the two roundings of the final sum
    (v + pos) + qrt: u |v + pos| + u |v + pos + qrt| <= u (2 |v| + 2 |pos| + |qrt|) -- v and pos pass through both
    roundings, which a bound of u |term| per addend leaves out.  The padded columns are exactly 0"""
    B, N, S, max_scale = 2, 3, 4, 518.0
    rows, D = B * N * S, 3 * L + 4
    ldx = (D + 31) // 32 * 32
    g = _rng(1500 + L)
    c = np.repeat(g.uniform(50, 450, (B * N, 1, 2)), S, axis=1) + g.uniform(-20, 20, (B * N, S, 2))
    coords = c.reshape(rows, 2).astype(np.float32)
    fcorr, fcv = _dev(g.standard_normal((rows, L)))
    tfeat, tfv = _dev(g.standard_normal((rows, L)))
    pos, posv = _dev(g.standard_normal((B * N, D)))
    qrt, qrtv = _dev(g.standard_normal((2, D)))
    ref, mag, trig = R.track_input(coords, fcv, tfv, posv, qrtv, S, L, ldx, max_scale)
    x = Guarded(torch.float32, (rows, ldx))
    ops.track_input(torch.from_numpy(coords).cuda(), fcorr, tfeat, pos, qrt, x.t, S, L, ldx, max_scale)
    x.check()
    _check(f"track_input L={L}", _np(x.t), ref, 4 * U * trig + U * mag)
    assert not x.t[:, D:].cpu().contiguous().view(torch.int32).any(), "padded columns must be exactly 0"


@pytest.mark.parametrize("want_pred", [False, True])
def test_track_coord_update(want_pred):
    B, N, S, L, stride = 2, 3, 4, 64, 2.0
    rows, ldd = B * N * S, L + 2
    g = _rng(1600)
    c0 = g.uniform(0, 200, (rows, 2)).astype(np.float32)
    delta = g.standard_normal((rows, ldd)).astype(np.float32)
    query = g.uniform(0, 200, (B * N, 2)).astype(np.float32)
    coords = Guarded(torch.float32, (rows, 2))
    coords.t.copy_(torch.from_numpy(c0))
    pred = Guarded(torch.float32, (B, S, N, 2)) if want_pred else None
    ops.track_coord_update_(coords.t, torch.from_numpy(delta).cuda(), ldd, torch.from_numpy(query).cuda(), N, S, stride,
                            pred=pred.t if want_pred else None)
    coords.check()
    refc, refp = R.track_coord_update(c0, delta, query, N, S, stride, want_pred)
    got = coords.t.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), refc.view(np.uint32))
    assert np.array_equal(got.reshape(B * N, S, 2)[:, 0].view(np.uint32), query.view(np.uint32)), "row s = 0 is the query"
    if want_pred:
        pred.check()
        assert np.array_equal(pred.t.cpu().numpy().view(np.uint32), refp.view(np.uint32))


def test_track_init_repeat_rows_bns_to_bsn():
    B, N, S, C = 2, 3, 4, 5
    g = _rng(1700)
    q = g.uniform(0, 500, (B * N, 2)).astype(np.float32)
    coords, qs = Guarded(torch.float32, (B * N, S, 2)), Guarded(torch.float32, (B * N, 2))
    ops.track_init(torch.from_numpy(q).cuda(), coords.t, qs.t, S, 2.0)
    coords.check(), qs.check()
    refc, refq = R.track_init(q, S, 2.0)
    assert np.array_equal(coords.t.cpu().numpy().view(np.uint32), refc.view(np.uint32))
    assert np.array_equal(qs.t.cpu().numpy().view(np.uint32), refq.view(np.uint32))

    src = g.standard_normal((B * N, C)).astype(np.float32)
    rep = Guarded(torch.float32, (B * N, S, C))
    ops.track_repeat_rows(torch.from_numpy(src).cuda(), S, out=rep.t)
    rep.check()
    assert np.array_equal(rep.t.cpu().numpy(), np.repeat(src[:, None], S, axis=1))

    v = g.standard_normal((B, N, S)).astype(np.float32)
    tr = Guarded(torch.float32, (B, S, N))
    ops.track_bns_to_bsn(torch.from_numpy(v).cuda(), out=tr.t)
    tr.check()
    assert np.array_equal(tr.t.cpu().numpy(), v.transpose(0, 2, 1))


# ------------------------------------------------------------------------------------------------------------------
# rejections: real, correctly sized buffers; only the named scalar is bad
# ------------------------------------------------------------------------------------------------------------------
def test_resize_rejects_too_many_rows():
    x = torch.zeros((65536, 1, 1, 4), device="cuda")
    out = Guarded(torch.float32, (65536, 1, 1, 4))
    with pytest.raises(_lib.SkimiError, match="65536"):
        ops.resize_bilinear(x, 1, 1, out=out.t)
    torch.cuda.synchronize()
    assert (out.full.cpu() == 0xFF).all()


def test_bad_arguments_are_rejected():
    """one rejected scalar per wrapper, through the return code and skimi_last_error"""
    L = _lib.lib()
    f = lambda *s: torch.zeros(s, device="cuda")                                   # noqa: E731
    h = lambda *s: torch.zeros(s, device="cuda", dtype=torch.int16)                # noqa: E731
    p = _lib.ptr
    a, b, c, d, e, o = f(4096), f(4096), f(4096), f(4096), f(4096), f(4096)
    F32 = _lib.F32
    calls = {
        "skimi_resize_bilinear": lambda: L.skimi_resize_bilinear(p(a), p(o), F32, F32, 2, 3, 5, 7, 12, 6, None, None, None, None, 0.0, None),        # C % 4
        "skimi_resize_bilinear_planes": lambda: L.skimi_resize_bilinear_planes(p(a), p(h(8192)), 2, 3, 5, 4, 4, 16, None, None, 1, None, None),     # records, C % 32
        "skimi_add_uv_pos": lambda: L.skimi_add_uv_pos(p(a), F32, p(b), p(c), 2, 3, 5, 12, None),                                                   # C % 8
        "skimi_add_uv_pos_records": lambda: L.skimi_add_uv_pos_records(p(a), p(b), p(c), 2, 3, 5, 48, p(h(8192)), None),                            # C % 32
        "skimi_dpt_out": lambda: L.skimi_dpt_out(p(a), F32, p(b), p(c), 3, p(o), p(d), 16, 0, None),                                                # n_out
        "skimi_patch_gather": lambda: L.skimi_patch_gather(p(a), p(o), F32, 1, 8, 12, 4, 40, None),                                                 # Kp < 3 p^2
        "skimi_adaln": lambda: L.skimi_adaln(p(a), p(b), p(c), p(o), 0, 8, None),                                                                   # rows
        "skimi_pose_update": lambda: L.skimi_pose_update(p(a), p(b), p(o), -1, 1, None),                                                            # rows
        "skimi_special_tokens": lambda: L.skimi_special_tokens(p(a), p(b), 4, 2, 7, 9, 8, None),                                                    # n > P
        "skimi_track_avgpool2": lambda: L.skimi_track_avgpool2(p(a), p(o), 2, 6, 8, 0, None),                                                       # C
        "skimi_track_sample_border": lambda: L.skimi_track_sample_border(p(a), 5 * 9 * 3 - 1, p(b), 2, p(o), 2, 8, 5, 9, 3, None),                  # img_stride
        "skimi_track_corr_sample": lambda: L.skimi_track_corr_sample(p(a), p(b), p(c), p(o), 12, 3, 2, 4, 4, 16, 1, 0, 17, 9, None),                # ldo
        "skimi_track_pos_embed_sample": lambda: L.skimi_track_pos_embed_sample(p(a), 2, p(o), 6, 5, 9, 198, None),                                  # D % 4
        "skimi_track_input": lambda: L.skimi_track_input(p(a), p(b), p(c), p(d), p(e), p(o), 8, 4, 64, 195, 518.0, None),                           # ldx
        "skimi_track_coord_update": lambda: L.skimi_track_coord_update(p(a), p(b), 1, p(c), None, 24, 3, 4, 2.0, None),                             # ldd
        "skimi_track_init": lambda: L.skimi_track_init(p(a), p(o), p(b), 6, 0, 2.0, None),                                                          # S
        "skimi_track_repeat_rows": lambda: L.skimi_track_repeat_rows(p(a), p(o), 6, 4, -5, None),                                                   # C
        "skimi_track_bns_to_bsn": lambda: L.skimi_track_bns_to_bsn(p(a), p(o), 2, 0, 4, None),                                                      # N
    }
    header = {n for n in _lib.exported_symbols() if n.startswith(("skimi_track_", "skimi_resize_", "skimi_add_uv", "skimi_dpt_out",
                                                                  "skimi_patch_gather", "skimi_adaln", "skimi_pose_update",
                                                                  "skimi_special_tokens"))}
    assert header == set(calls)
    for name, call in calls.items():
        assert call() != 0, f"{name} accepted a bad argument"
        assert L.skimi_last_error(), name
    # and a null buffer
    assert L.skimi_track_avgpool2(None, p(o), 2, 6, 8, 3, None) != 0 and b"null" in L.skimi_last_error()
    torch.cuda.synchronize()
    assert not o.any(), "a rejected call wrote its output"
