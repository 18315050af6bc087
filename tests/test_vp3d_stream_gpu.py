"""GPU: every kernel of the small-batch VideoPose3D streaming path (csrc/vp3d_stream.hip, csrc/vp3d_dense.hip), one launch
at a time through its C entry (include/skimi.h, "VideoPose3D small-batch streaming layers"), against the float64
restatement tests/vp3d_stream_restated.py.  Every case asserts the plan it ran through skimi_vp3d_last_plan.

Exact cases.  Operands a + b 2^-9 (a a small integer, b in {-1, 0, 1}) split into hi = a, lo = b 2^-9; every kept
product is a multiple of 2^-9 and the absolute sum stays below 2^15, so all partial sums fit fp32's 24 bits, every
summation order is exact and the kernel must equal reference A (Whi Xhi + Whi Xlo + Wlo Xhi) bit for bit -- which also
pins the dropped term to lo x lo: reference B (the unsplit product) differs there by construction.

Random data.  Against reference A the kernel differs only by the rounding of its fp32 additions: with S the absolute
sum of the kept terms, the bias and the residual and n the additions on an output's longest path,
    |kernel - A| <= gamma_n S,   gamma_n = n u / (1 - n u),   u = 2^-24.
Counted from the kernels: a wave accumulates 3 products for each of the 32 elements of each of its K slices (at most
3 K if one wave had all of K), the K-partials are then added up -- NW TAPS additions in vp3d_conv_kernel (v starts
at zero), 7 in vp3d_mm_kernel and vp3d_win_kernel -- then the bias and the residual: the longest path has at most
n = 3 K + NW TAPS + 3 additions (TAPS = 1 outside vp3d_conv_kernel), the issue's conservative count, used as it is.
Against reference B: with p = 8 significant bits bf16's unit roundoff is 2^-8, so |x - hi| <= 2^-8 |x|, lo = bf16(x - hi)
leaves |x - hi - lo| <= 2^-16 |x|, and |lo| <= 2^-8 (1 + 2^-8) |x|.  Then
    w x - (Whi Xhi + Whi Xlo + Wlo Xhi) = (w - Whi - Wlo) x + (Whi + Wlo) (x - Xhi - Xlo) + Wlo Xlo,
three terms of at most 2^-16 |w| |x| each to first order: |A - B| <= 3 * 2^-16 sum |w| |x|, added to the bound above.
(The second-order surplus, (2^-7 + 2^-16) 2^-16 |w| |x| if all three were extreme at once, is 2^-23 sum |w| |x|.)
Bounds come from the references alone.  Each test prints `RATIO <kernel> <worst error / bound>`; the worst figures of
an MI355X run are in profiles/vp3d_stream_unit.md.
"""
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import vp3d_stream_restated as R  # noqa: E402

from skiing_analysis_pytorch_amd import _lib, vp3d, weights as W  # noqa: E402
from skiing_analysis_pytorch_amd._lib import PREC_BF16X3  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
CSRC = Path(_lib.__file__).resolve().parent / "csrc"
CONV, MM, WIN, EMFMA, EVALU = _lib.VP3D_CONV, _lib.VP3D_MM, _lib.VP3D_WIN, _lib.VP3D_EXPAND_MFMA, _lib.VP3D_EXPAND_VALU
U = R.U
SENTINEL = 0x7FC1      # a bf16 NaN no kernel writes: untouched record halves keep it


# ---- data --------------------------------------------------------------------------------------------------------
def _rng(*key):
    return np.random.default_rng([abs(int(k)) for k in key])


def exact_values(g, shape, amax=3):
    """a + b 2^-9, a in +-{1..amax}, b in {-1, 0, 1}, one in eight an exact zero"""
    a = g.integers(1, amax + 1, shape) * g.choice([-1, 1], shape)
    b = g.integers(-1, 2, shape)
    v = a + b * 2.0 ** -9
    v[g.random(shape) < 0.125] = 0.0
    return v.astype(np.float32)


def small_ints(g, shape, lim=4):
    return g.integers(-lim, lim + 1, shape).astype(np.float32)


def scaled_normal(g, shape):
    """normal values with a scale per channel (last axis) spread over 2^+-6"""
    return (g.standard_normal(shape) * 2.0 ** g.uniform(-6, 6, shape[-1])).astype(np.float32)


# ---- one launch ----------------------------------------------------------------------------------------------------
class Layer:
    """One layer's operands.  kind: conv / mm / win share the conv arithmetic; emfma / evalu are expand_conv."""

    def __init__(self, Wt, X, bias, N=None, Npad=None, dil=1, relu=True, resid=None, resid_off=0):
        self.Wt, self.X, self.bias = Wt, X, bias          # [N, taps, C], [B, Lin, C], [N]
        self.N, self.taps, self.C = Wt.shape
        assert N in (None, self.N)
        self.Npad = Npad or -(-self.N // 16) * 16
        self.B, self.Lin = X.shape[:2]
        self.dil, self.relu, self.resid, self.resid_off = dil, relu, resid, resid_off
        self.Lout = self.Lin - (self.taps - 1) * dil
        self.M = self.B * self.Lout

    def reference(self):
        r = R.conv(self.Wt, self.X, self.bias, self.dil, self.relu, self.resid, self.resid_off)
        return {k: v.reshape(self.M, self.N) for k, v in r.items()}


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def launch(kind, L, force=None, ldo=None, f32=True, rec=None):
    """Runs layer L on kernel family `kind`; returns (out [M, N] fp32 or None, (hi, lo) [M, N] or None, plan).
    The fp32 buffer is NaN-filled with a guard row on each side, the records sentinel-filled with a guard tile on each
    side: everything the kernel must not touch is checked here."""
    N, M = L.N, L.M
    rec = (N % 32 == 0) if rec is None else rec
    ldo = ldo or N
    bias = _cuda(L.bias)
    obuf = torch.full((M + 2, ldo), float("nan"), dtype=torch.float32, device=DEV) if f32 else None
    tiles = -(-M // 16)
    rbuf = torch.full(((tiles + 2) * (N // 32) * 1024,), SENTINEL, dtype=torch.int16, device=DEV) if rec else None
    out_ptr = obuf[1:] if f32 else None
    rec_ptr = rbuf[(N // 32) * 1024:] if rec else None
    if kind in ("emfma", "evalu"):
        assert f32 and rec and L.dil == 1 and L.relu and L.resid is None
        Cin, K = L.C, L.taps * L.C
        x = _cuda(L.X)
        if kind == "emfma":
            Kpad = -(-K // 32) * 32
            wp = np.zeros((N, Kpad), np.float32)
            wp[:, :K] = L.Wt.reshape(N, K)
            w, ldw = vp3d.pack_weights(torch.from_numpy(wp), N, DEV), Kpad
        else:
            w, ldw = _cuda(L.Wt.reshape(N, K)), K
        vp3d.stream_expand(x, w, ldw, bias, out_ptr, rec_ptr, L.B, L.Lin, Cin, L.taps, N, valu=kind == "evalu", force_ms=force or 0)
    else:
        wrec = vp3d.pack_weights(torch.from_numpy(L.Wt.reshape(N, -1)), L.Npad, DEV)
        xrec = _cuda(R.pack(L.X.reshape(L.B * L.Lin, L.C)).view(np.int16).reshape(-1))
        if kind == "win":
            assert L.dil == 1 and L.relu and L.resid is None
            vp3d.stream_win(wrec, L.Npad, xrec, bias, out_ptr, ldo, rec_ptr, L.B, L.Lin, L.C, L.taps, N, force=force or (0, 0))
        else:
            resid = None if L.resid is None else _cuda(L.resid)
            vp3d.stream_mm(wrec, L.Npad, xrec, bias, out_ptr, ldo, rec_ptr, L.B, L.Lin, L.C, L.taps, L.dil, N, relu=L.relu,
                           resid=resid, resid_L=0 if L.resid is None else L.resid.shape[1], resid_off=L.resid_off,
                           force=force or (0, 0, 0, 0))
    if DEV == "cuda":
        torch.cuda.synchronize()
    plan = vp3d.last_plan()
    out = halves = None
    if f32:
        o = obuf.cpu().numpy()
        assert np.isnan(o[0]).all() and np.isnan(o[-1]).all(), "a guard row of the fp32 output was written"
        assert np.isnan(o[1:-1, N:]).all(), "columns >= N of the padded fp32 output were written"
        out = o[1:-1, :N]
        assert not np.isnan(out).any(), "an output element was not written"
    if rec:
        r = rbuf.cpu().numpy().view(np.uint16)
        g = (N // 32) * 1024
        assert (r[:g] == SENTINEL).all() and (r[-g:] == SENTINEL).all(), "a guard tile of the records was written"
        body = r[g:-g]
        t = body.reshape(tiles, N // 32, 2, 4, 16, 8).transpose(2, 0, 4, 1, 3, 5).reshape(2, tiles * 16, N)   # [hi | lo][row][n]
        assert (t[:, :M] != SENTINEL).all(), "a record element was not written"
        halves = R.unpack(body, M, N)
    return out, halves, plan


def n_adds(kind, K, nw=8, taps_t=1):
    """additions on an output's longest path (module docstring); the VALU expand is K sequential FMAs + the bias"""
    return 3 * K + nw * taps_t + 3


def gamma(n):
    return n * U / (1 - n * U)


def check(kind, L, out, halves, plan, exact, ref=None):
    """The comparison every case shares (ref: the reference of the rows given, else of the whole layer).  Returns the
    worst error / bound against reference A (B for the VALU expand)."""
    ref = ref or L.reference()
    K = L.taps * L.C if kind == "evalu" else -(-L.taps * L.C // 32) * 32
    if out is not None and halves is not None:      # the records are the split of the fp32 value, whatever it is
        eh, el = R.split(out)
        assert np.array_equal(halves[0].view(np.uint32), eh.view(np.uint32)), "records: hi is not bf16(out)"
        assert np.array_equal(halves[1].view(np.uint32), el.view(np.uint32)), "records: lo is not bf16(out - hi)"
    if exact:
        assert (ref["SA"] < 2.0 ** 15).all(), "the case leaves the range in which fp32 sums are exact"
        A32 = ref["A"].astype(np.float32)
        assert np.array_equal(A32.astype(np.float64), ref["A"])
        if kind == "evalu":     # integers: sequential fp32 FMA is exact, A = B
            assert np.array_equal(ref["A"], ref["B"])
        else:
            assert (ref["A"] != ref["B"]).any(), "the case does not tell the dropped lo x lo term from a kept one"
        if out is not None:
            bad = np.argwhere(out != A32)
            assert bad.size == 0, f"{len(bad)} of {out.size} outputs differ from reference A, first {bad[:4].tolist()}: " \
                                  f"{out[tuple(bad[0])]} vs {A32[tuple(bad[0])]}"
        else:
            eh, el = R.split(A32)
            assert np.array_equal(halves[0], eh) and np.array_equal(halves[1], el)
        return 0.0
    if kind == "evalu":
        bound = (K + 2) * U * (ref["SB"] + np.abs(L.bias.astype(np.float64))) + 1e-300
        err = np.abs(out.astype(np.float64) - ref["B"])
        ratio = float((err / bound).max())
        print(f"RATIO {kind} vsB {ratio:.4f}")
        assert ratio <= 1.0
        return ratio
    n = n_adds(kind, K, plan[4], plan[3] if kind == "conv" else 1)
    bA = gamma(n) * ref["SA"] + 1e-300
    if out is not None:
        got, slack = out.astype(np.float64), 0.0
    else:       # records only: hi + lo is within 2^-16 of the fp32 value the kernel split
        got = halves[0].astype(np.float64) + halves[1].astype(np.float64)
        slack = 2.0 ** -16 * (np.abs(ref["A"]) + bA)
    rA = float((np.abs(got - ref["A"]) / (bA + slack)).max())
    rB = float((np.abs(got - ref["B"]) / (bA + slack + 3 * 2.0 ** -16 * ref["SB"])).max())
    print(f"RATIO {kind} K={K} vsA {rA:.4f} vsB {rB:.4f}")
    assert rA <= 1.0, f"error / bound against reference A: {rA}"
    assert rB <= 1.0, f"error / bound against reference B: {rB}"
    return rA


def make_layer(seed, N, C, taps, dil, B, Lin, exact, Npad=None, relu=True, resid_L=0, resid_off=0, amax=3, expand=False):
    g = _rng(seed, N, C, taps, dil, B, Lin, int(exact))
    if exact:
        Wt, X = exact_values(g, (N, taps, C), amax), exact_values(g, (B, Lin, C), amax)
        bias = small_ints(g, N)
        resid = small_ints(g, (B, resid_L, N)) if resid_L else None
    else:
        Wt, X = scaled_normal(g, (N, taps, C)), scaled_normal(g, (B, Lin, C))
        bias = g.standard_normal(N).astype(np.float32)
        resid = g.standard_normal((B, resid_L, N)).astype(np.float32) if resid_L else None
    return Layer(Wt, X, bias, Npad=Npad, dil=dil, relu=relu, resid=resid, resid_off=resid_off)


def both(kind, force, expect, **kw):
    """one exact and one random launch of a case; both must run the expected plan"""
    worst = 0.0
    for exact in (True, False):
        if kind == "evalu" and exact:       # integers: exact under sequential FMA
            g = _rng(7, kw["N"], kw["C"])
            L = Layer(small_ints(g, (kw["N"], kw["taps"], kw["C"]), 3), small_ints(g, (kw["B"], kw["Lin"], kw["C"]), 3),
                      small_ints(g, kw["N"]))
        else:
            L = make_layer(11, exact=exact, **kw)
        out, halves, plan = launch(kind, L, force)
        if expect is not None:
            assert plan == expect, f"plan {plan}, expected {expect}"
        worst = max(worst, check(kind, L, out, halves, plan, exact))
    return worst


# ---- 5a: every instantiation ---------------------------------------------------------------------------------------
def ladder_rows():
    """The launch ladders, read from the sources: every row must have a case below."""
    s, d = (CSRC / "vp3d_stream.hip").read_text(), (CSRC / "vp3d_dense.hip").read_text()
    rows = []
    for ct, rt, taps in re.findall(r"SKIMI_VP3D_CONV\((\d+), (\d+), (\d+)\)", s):
        rows += [("conv", int(ct), int(rt), int(taps), 8), ("conv", int(ct), int(rt), int(taps), 4)]
    rows += [("mm", int(ct), int(rt)) for ct, rt in re.findall(r"SKIMI_VP3D_CASE\((\d+), (\d+)\)", s)]
    rows += [("win", int(ta), int(rt)) for ta, rt in re.findall(r"SKIMI_VP3D_WIN\((\d+), (\d+)\)", d)]
    rows += [("emfma", int(rt)) for rt in re.findall(r"launch_conv<32, (\d+), 1, 1>\(q", s)]
    rows += [("evalu",)] * len(re.findall(r"hipLaunchKernelGGL\(vp3d_expand_kernel,", s))
    return rows


def instantiation_case(row):
    """(kind, force, expected plan, layer arguments) of a ladder row.  Every case: B = 2, R = 16 RT - 7 (the last row
    tile is partial), Lout not a multiple of the row splits, B Lin not a multiple of 16 (record tiles straddle the
    clips), two channel tiles; for mm three row splits of 2 Lout rows, so the middle workgroup straddles the clips."""
    kind = row[0]
    if kind == "conv":
        _, ct, rt, taps, nw = row
        halo = 4 if taps == 3 else 0
        Rr = 16 * rt - 3 - halo
        Lout, N = 2 * Rr - 1, 2 * ct
        assert -(-(Rr + halo) // 16) == rt and Rr % 16 and Lout % 2 and (2 * (Lout + halo)) % 16
        return kind, (CONV, ct, nw, 2), (CONV, ct, rt, taps, nw, 2, Rr, 2 * 2 * 2), \
            dict(N=N, C=96, taps=taps, dil=2, B=2, Lin=Lout + halo)
    if kind == "mm":
        _, ct, rt = row
        Rr = 16 * rt - 7
        Mr = 3 * Rr - 1
        Lout, N = Mr // 2, 2 * ct
        assert Mr % 2 == 0 and Mr % 3 and (2 * (Lout + 4)) % 16 and Rr < Lout < 2 * Rr
        return kind, (MM, ct, 0, 3), (MM, ct, rt, 3, 8, 3, Rr, 2 * 3), dict(N=N, C=96, taps=3, dil=2, B=2, Lin=Lout + 4)
    if kind == "win":
        _, ta, rt = row
        Rr = 16 * rt - 7
        Lout, N = 2 * Rr - 1, 32 * ta
        assert (2 * (Lout + 4)) % 16
        return kind, (ta, 2), (WIN, 16 * ta, rt, 5, 8, 2, Rr, 2 * 2 * 2), dict(N=N, C=96, taps=5, dil=1, B=2, Lin=Lout + 4)
    if kind == "emfma":
        rt = row[1]
        Rr = 16 * rt - 7
        Lout = 2 * Rr - 1
        return kind, 2, (EMFMA, 32, rt, 1, 8, 2, Rr, 2 * 2 * 2), dict(N=64, C=34, taps=3, dil=1, B=2, Lin=Lout + 2)
    return kind, 3, (EVALU, 32, 0, 3, 4, 3, 14, 2 * 3), dict(N=64, C=34, taps=3, dil=1, B=2, Lin=23)


# the 61 instantiations, written out: 30 conv, 9 mm, 16 window, 5 MFMA expand, the VALU expand
INSTANTIATIONS = ([("conv", 16, rt, 3, nw) for rt in range(1, 6) for nw in (8, 4)] +
                  [("conv", ct, rt, 1, nw) for ct in (16, 32) for rt in range(1, 6) for nw in (8, 4)] +
                  [("mm", 16, rt) for rt in range(1, 6)] + [("mm", 32, rt) for rt in range(1, 5)] +
                  [("win", ta, rt) for ta in (1, 2) for rt in range(1, 9)] +
                  [("emfma", rt) for rt in range(1, 6)] + [("evalu",)])


def _id(row):
    return "-".join(str(v) for v in row)


def test_ladder_is_complete():
    """Every row of the launch ladders in the sources has a case, and nothing else is listed."""
    rows = ladder_rows()
    assert len(rows) == 61 and len(set(rows)) == 61, len(rows)
    assert len(INSTANTIATIONS) == 61
    assert sorted(rows) == sorted(INSTANTIATIONS)


@pytest.mark.parametrize("row", INSTANTIATIONS, ids=_id)
def test_every_instantiation(row):
    """Forced onto its instantiation at a small ragged shape: the plan is the forced one, the exact case is bit-equal
    to reference A, the random case inside both bounds."""
    kind, force, expect, kw = instantiation_case(row)
    both(kind, force, expect, **kw)


# ---- 5b: the planner's own choices ------------------------------------------------------------------------------------
# (Npad, C, taps, dil, B, Lin) -> the plan of this tree's planner
PLANNED = [
    ((16, 32, 3, 9, 1, 19), (CONV, 16, 2, 3, 8, 1, 1, 1)),
    ((1024, 32, 3, 1, 6, 18), (CONV, 16, 2, 3, 4, 1, 16, 384)),
    ((512, 32, 1, 1, 32, 80), (CONV, 32, 5, 1, 4, 1, 80, 512)),
    ((16, 32, 3, 27, 1, 55), (MM, 16, 1, 3, 8, 1, 1, 1)),
    ((1024, 32, 1, 1, 6, 80), (MM, 32, 4, 1, 8, 8, 60, 256)),
    ((32, 96, 5, 1, 2, 23), (MM, 16, 1, 5, 8, 38, 1, 76)),          # filter width 5: no conv instantiation
    ((32, 96, 3, 41, 2, 101), (MM, 16, 1, 3, 8, 38, 1, 76)),        # a halo of 82 rows does not fit five row tiles
    ((64, 96, 1, 1, 2, 37), (CONV, 16, 1, 1, 8, 32, 2, 256)),
    ((48, 96, 1, 1, 2, 21), (CONV, 16, 1, 1, 8, 21, 1, 126)),
    ((64, 96, 3, 3, 2, 45), (CONV, 16, 1, 3, 8, 32, 2, 256)),
    ((64, 32, 1, 1, 3, 100), (CONV, 16, 1, 1, 8, 21, 5, 252)),
    ((512, 32, 1, 1, 2, 200), (CONV, 32, 2, 1, 8, 8, 25, 256)),
    ((1024, 32, 1, 1, 2, 75), (CONV, 16, 3, 1, 8, 2, 38, 256)),
]


@pytest.mark.parametrize("shape,expect", PLANNED, ids=[_id(s) for s, _ in PLANNED])
def test_planner_choice(shape, expect):
    Npad, C, taps, dil, B, Lin = shape
    L = make_layer(21, Npad, C, taps, dil, B, Lin, exact=True)
    out, halves, plan = launch("mm", L)
    assert plan == expect
    check("conv" if plan[0] == CONV else "mm", L, out, halves, plan, True)


# an RF-27 forward of 269 frames at C = 1024: (name, family of the entry, layer arguments, plan at B = 1, at B = 2)
PRODUCTION = [
    ("expand", "emfma", dict(N=1024, C=34, taps=3, dil=1, Lin=269), (EMFMA, 32, 3, 1, 8, 8, 34, 256), (EMFMA, 32, 5, 1, 8, 4, 67, 256)),
    ("conv_d3", "mm", dict(N=1024, C=1024, taps=3, dil=3, Lin=267), (CONV, 16, 5, 3, 8, 4, 66, 256), (CONV, 16, 5, 3, 4, 4, 66, 512)),
    ("conv_1x1_a", "mm", dict(N=1024, C=1024, taps=1, dil=1, Lin=261), (CONV, 32, 3, 1, 8, 8, 33, 256), (CONV, 32, 5, 1, 8, 4, 66, 256)),
    ("conv_d9", "mm", dict(N=1024, C=1024, taps=3, dil=9, Lin=261), (CONV, 16, 5, 3, 8, 4, 61, 256), (CONV, 16, 5, 3, 4, 4, 61, 512)),
    ("conv_1x1_b", "mm", dict(N=1024, C=1024, taps=1, dil=1, Lin=243), (CONV, 32, 2, 1, 8, 8, 31, 256), (CONV, 32, 4, 1, 8, 4, 61, 256)),
    ("shrink", "mm", dict(N=51, C=1024, taps=1, dil=1, Lin=243), (CONV, 16, 1, 1, 8, 64, 4, 256), (CONV, 16, 1, 1, 8, 32, 8, 256)),
]


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("name,kind,kw,plan1,plan2", PRODUCTION, ids=[p[0] for p in PRODUCTION])
def test_production_shapes(name, kind, kw, plan1, plan2, B):
    """The six layers of the application's forward, planned, exact data (|a| <= 3 at K = 3072), checked on 24 rows
    (first, last, the rows around the clip boundary and a spread): the reference of a whole layer is seconds of float64."""
    L = make_layer(31, B=B, exact=True, relu=name != "shrink", **kw)
    out, halves, plan = launch(kind, L)
    assert plan == (plan1 if B == 1 else plan2)
    rows = np.unique(np.concatenate([[0, 1, 15, 16, L.Lout - 1, L.M - L.Lout, L.M - 1], _rng(B).integers(0, L.M, 17)]))
    ref = R.contract_rows(L.Wt, L.X, L.bias, L.dil, L.relu, rows)
    check("conv" if plan[0] == CONV else kind, L, out[rows], None if halves is None else (halves[0][rows], halves[1][rows]),
          plan, True, ref=ref)


# ---- 5c: the ends of the K loop ----------------------------------------------------------------------------------------
def wave_counts(S, nw):
    """slices per wave: wave w owns [w S / nw, (w + 1) S / nw)"""
    return [(w + 1) * S // nw - w * S // nw for w in range(nw)]


KLOOP_CONV = [(8, 32, 1), (8, 96, 1), (8, 384, 1), (8, 768, 1), (8, 1280, 1), (8, 384, 3),
              (4, 32, 1), (4, 160, 1), (4, 384, 1), (4, 768, 1), (4, 160, 3)]
KLOOP_MM = [(32, 1), (96, 3), (160, 3), (384, 1), (384, 3), (768, 1), (768, 3), (1280, 1)]


def test_kloop_cases_cover_the_ends():
    for nw in (8, 4):
        sets = [wave_counts(C // 32, nw) for n, C, _ in KLOOP_CONV if n == nw]
        seen = set().union(*sets)
        assert {0, 1, 2, 3} <= seen and max(seen) >= 5, (nw, seen)
        assert any(len(set(s)) > 1 and min(s) > 0 for s in sets), "no case with unequal non-empty waves"
    sets = [wave_counts(t * C // 32, 8) for C, t in KLOOP_MM]
    seen = set().union(*sets)
    assert {0, 1, 2, 3} <= seen and max(seen) >= 5 and {c % 3 for c in seen if c} == {0, 1, 2}, seen
    assert any(len(set(s)) > 1 and min(s) > 0 for s in sets)


@pytest.mark.parametrize("nw,C,taps", KLOOP_CONV)
def test_kloop_conv(nw, C, taps):
    """vp3d_conv_kernel, depth 2: waves with 0, 1, 2, 3 and more slices, odd tails, unequal waves"""
    dil = 2 if taps == 3 else 1
    Lin = 21 + (taps - 1) * dil
    rt = -(-(21 + (taps - 1) * dil) // 16)
    both("conv", (CONV, 16, nw, 1), (CONV, 16, rt, taps, nw, 1, 21, 2), N=16, C=C, taps=taps, dil=dil, B=2, Lin=Lin)


@pytest.mark.parametrize("C,taps", KLOOP_MM)
def test_kloop_mm(C, taps):
    """vp3d_mm_kernel, depth 3: all residues of the slice count mod 3"""
    Lin = 11 + (taps - 1) * 2
    both("mm", (MM, 16, 0, 2), (MM, 16, 1, taps, 8, 2, 11, 2), N=16, C=C, taps=taps, dil=2, B=2, Lin=Lin)


@pytest.mark.parametrize("taps", [1, 3, 7, 8, 9, 19, 55])
def test_window_taps(taps):
    """the taps go round-robin over eight waves: 7, 8 and 9 are the boundaries; planned"""
    both("win", None, (WIN, 16, 1, taps, 8, 2, 11, 8), N=32, C=96, taps=taps, dil=1, B=2, Lin=20 + taps)


def test_window_too_wide_falls_back_to_mm():
    """taps so many that no window fits: 16 RT + taps - 1 rounded up to 16 exceeds VP3D_WIN_MAX_NR even at RT = 1"""
    d = (CSRC / "vp3d_dense.hip").read_text()
    su = int(re.search(r"VP3D_WIN_SU = (\d+);", d).group(1))
    assert "VP3D_WIN_MAX_NR = 64 * VP3D_WIN_SU" in d
    max_nr = 64 * su
    taps = max_nr - 16 + 2            # 16 + taps - 1 = max_nr + 1
    assert -(-(16 + taps - 2) // 16) * 16 <= max_nr < -(-(16 + taps - 1) // 16) * 16
    L = make_layer(41, 32, 32, taps, 1, 2, taps + 9, exact=True, amax=1)
    out, halves, plan = launch("win", L)
    assert plan[0] == MM and plan[3] == taps
    check("mm", L, out, halves, plan, True)
    # one tap fewer still has a window
    L = make_layer(41, 32, 32, taps - 1, 1, 2, taps + 8, exact=True, amax=1)
    out, halves, plan = launch("win", L)
    assert plan[0] == WIN and plan[2] == 1 and plan[3] == taps - 1
    check("win", L, out, halves, plan, True)


# ---- 5d: the epilogue --------------------------------------------------------------------------------------------------
EPI_KERNELS = {"conv8": ("conv", (CONV, 16, 8, 2)), "conv4": ("conv", (CONV, 16, 4, 2)), "mm": ("mm", (MM, 16, 0, 3)),
               "win": ("win", (1, 2))}


@pytest.mark.parametrize("kern", list(EPI_KERNELS))
@pytest.mark.parametrize("N,Npad,ldo", [(3, 16, 3), (6, 16, 6), (9, 16, 9), (36, 48, 36), (48, 48, 48), (51, 64, 51), (36, 48, 40),
                                        (51, 64, 52)])
def test_epilogue_narrow_output(kern, N, Npad, ldo):
    """c >= N, the clamped bias index, float4 against scalar-tail stores (ldo % 4 and c + 3 < N); fp32 output only.  The
    last two pad ldo: the columns N .. ldo - 1 must stay untouched (checked in launch())."""
    kind, force = EPI_KERNELS[kern]
    for exact in (True, False):
        L = make_layer(51, N, 96, 3, 1, 2, 23, exact=exact, Npad=Npad)
        out, halves, plan = launch(kind, L, force, ldo=ldo, rec=False)
        assert plan[0] == {"conv": CONV, "mm": MM, "win": WIN}[kind]
        check(kind, L, out, halves, plan, exact)


@pytest.mark.parametrize("kern", list(EPI_KERNELS))
@pytest.mark.parametrize("mode", ["records", "fp32", "both"])
def test_epilogue_output_modes(kern, mode):
    kind, force = EPI_KERNELS[kern]
    for exact in (True, False):
        L = make_layer(52, 64, 96, 3, 1, 2, 23, exact=exact)
        out, halves, plan = launch(kind, L, force, f32=mode != "records", rec=mode != "fp32")
        assert (out is None) == (mode == "records") and (halves is None) == (mode == "fp32")
        check(kind, L, out, halves, plan, exact)


@pytest.mark.parametrize("kern", ["conv8", "conv4", "mm"])
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("resid", [None, 0, 1, "causal"])
def test_epilogue_relu_and_residual(kern, relu, resid):
    """x = res + relu(conv): the residual row is b resid_L + l + resid_off with resid_L > Lout; "causal": pad + shift of
    a causal block (fw 3 at dilation 3: pad 3, shift 3)"""
    kind, force = EPI_KERNELS[kern]
    off = {None: 0, 0: 0, 1: 1, "causal": 6}[resid]
    for exact in (True, False):
        L = make_layer(53, 96, 96, 3, 3, 2, 25, exact=exact, relu=relu, resid_L=0 if resid is None else 27, resid_off=off)
        assert L.resid is None or L.resid.shape[1] >= L.Lout + off and L.resid.shape[1] > L.Lout
        out, halves, plan = launch(kind, L, force)
        check(kind, L, out, halves, plan, exact)
        if not relu and not exact:
            assert (out < 0).any()


# ---- 5f: random data at K = 96 and K = 3 * 1024 ------------------------------------------------------------------------
@pytest.mark.parametrize("kern", ["conv8", "conv4", "mm", "win"])
@pytest.mark.parametrize("C", [32, 1024])
def test_random_data(kern, C):
    kind, force = EPI_KERNELS[kern]
    L = make_layer(61, 32, C, 3, 1, 2, 25, exact=False)
    out, halves, plan = launch(kind, L, force)
    check(kind, L, out, halves, plan, False)


@pytest.mark.parametrize("Cin", [32, 34])
@pytest.mark.parametrize("kind", ["emfma", "evalu"])
def test_random_data_expand(kind, Cin):
    """Cin = 32: kvalid == Kpad = 96; Cin = 34: kvalid = 102 < Kpad = 128 (the tail reads as zero)"""
    L = make_layer(62, 64, Cin, 3, 1, 2, 40, exact=False)
    out, halves, plan = launch(kind, L)
    assert plan[0] == (EMFMA if kind == "emfma" else EVALU)
    check(kind, L, out, halves, plan, False)
    Le = make_layer(62, 64, Cin, 3, 1, 2, 40, exact=True)
    if kind == "evalu":
        g = _rng(63, Cin)
        Le = Layer(small_ints(g, (64, 3, Cin), 3), small_ints(g, (2, 40, Cin), 3), small_ints(g, 64))
    out, halves, plan = launch(kind, Le)
    check(kind, Le, out, halves, plan, True)


# ---- 5g: invariance ----------------------------------------------------------------------------------------------------
def test_window_result_is_the_same_for_every_tiling():
    """vp3d_dense.hip's header: the accumulation order of an output is the same for every (TA, RT, msc) -- slice-major,
    the taps of a slice round-robin over the waves, the eight partials in wave order.  One random input through every
    feasible tiling (both TA, every msc from 1 to Lout = 120: RT 8, 4, 3, 2 and 1): fp32 and records bit-identical."""
    L = make_layer(71, 32, 96, 7, 1, 2, 126, exact=False)
    assert L.Lout == 120
    first, seen = None, set()
    for ta in (1, 2):
        for msc in range(1, L.Lout + 1):
            out, halves, plan = launch("win", L, (ta, msc))
            assert plan[:2] == (WIN, 16 * ta) and plan[5] == msc and plan[2] == -(-(-(-120 // msc)) // 16)
            seen.add((ta, plan[2]))
            if first is None:
                first = (out, halves)
                check("win", L, out, halves, plan, False)
            else:
                assert np.array_equal(out.view(np.uint32), first[0].view(np.uint32)), (ta, msc)
                assert np.array_equal(halves[0], first[1][0]) and np.array_equal(halves[1], first[1][1]), (ta, msc)
    assert seen == {(ta, rt) for ta in (1, 2) for rt in (1, 2, 3, 4, 8)}      # R = ceil(120 / msc): 120, 60, 40, 30, ...


@pytest.mark.parametrize("kern", ["conv8", "conv4", "mm"])
def test_two_runs_are_bit_identical(kern):
    kind, force = EPI_KERNELS[kern]
    L = make_layer(72, 64, 384, 3, 2, 2, 41, exact=False)
    a = launch(kind, L, force)
    b = launch(kind, L, force)
    assert a[2] == b[2]
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
    assert np.array_equal(a[1][0], b[1][0]) and np.array_equal(a[1][1], b[1][1])


@pytest.mark.parametrize("kern", ["conv8", "conv4", "mm", "win"])
def test_clip_of_a_batch_equals_its_own_launch(kern):
    """Every clip of a B = 3 launch against its B = 1 launch under the same forced (family, CT, NW).  The window kernel
    fixes the order of an output's additions whatever the grid (above).  vp3d_conv_kernel and vp3d_mm_kernel rotate the
    order in which a wave walks its K slices by the workgroup's index, which depends on the batch: there the order of
    an output is the same only while no wave owns more than one slice -- C = 96: three slices (nine for mm's three
    taps, over eight waves: the one wave with two slices rules mm out at taps 3, so mm runs one tap here)."""
    kind, force = EPI_KERNELS[kern]
    taps = 1 if kern == "mm" else 3
    if kern != "win":
        assert max(wave_counts(3, 4 if kern == "conv4" else 8)) <= 1
    L3 = make_layer(73, 32, 96, taps, 1, 3, 29, exact=False)
    force = force[:-1] + (0,)       # the planner's row split for each batch; (family, CT, NW) held
    out3, halves3, plan3 = launch(kind, L3, force)
    for b in range(3):
        L1 = Layer(L3.Wt, L3.X[b:b + 1], L3.bias)
        out1, halves1, plan1 = launch(kind, L1, force)
        assert plan1[:2] == plan3[:2] and plan1[4] == plan3[4]
        sl = slice(b * L3.Lout, (b + 1) * L3.Lout)
        assert np.array_equal(out3[sl].view(np.uint32), out1.view(np.uint32)), b
        assert np.array_equal(halves3[0][sl], halves1[0]) and np.array_equal(halves3[1][sl], halves1[1]), b


# ---- 5h: refusals ------------------------------------------------------------------------------------------------------
REFUSED_MM = [
    # (Npad, C, taps, dil, B, Lin), force, a piece of the message
    ((48, 32, 1, 1, 2, 21), (CONV, 32, 8, 1), "not a multiple of CT"),
    ((32, 32, 3, 1, 2, 21), (CONV, 32, 8, 1), "3 taps need CT 16"),
    ((32, 32, 5, 1, 2, 21), (CONV, 16, 8, 1), "1 or 3 taps"),
    ((32, 32, 3, 40, 2, 101), (CONV, 16, 8, 1), "halo of 80 rows"),
    ((32, 32, 3, 2, 2, 104), (CONV, 16, 8, 1), "row tiles"),                # R + halo = 104 rows: 7 tiles
    ((32, 32, 1, 1, 2, 100), (MM, 16, 0, 2), "row tiles"),                  # 100 rows per workgroup
    ((32, 32, 1, 1, 2, 100), (MM, 32, 0, 3), "at most 4 fit at CT 32"),     # 67 rows: 5 tiles
    ((32, 32, 1, 1, 2, 21), (CONV, 16, 8, 22), "exceeds Lout"),
    ((32, 32, 1, 1, 2, 21), (MM, 16, 0, 43), "exceeds the 42 rows"),
    ((32, 32, 1, 1, 2, 21), (CONV, 16, 2, 1), "NW 2"),
    ((32, 32, 1, 1, 2, 21), (MM, 16, 4, 1), "8 waves"),
    ((32, 32, 1, 1, 2, 21), (CONV, 24, 8, 1), "CT 24"),
    ((32, 32, 1, 1, 2, 21), (7, 16, 8, 1), "family 7"),
]


def _refused(call, piece):
    before = vp3d.last_plan()
    with pytest.raises(_lib.SkimiError) as e:
        call()
    assert piece in str(e.value), str(e.value)
    assert "unsupported tiling" not in str(e.value)
    assert vp3d.last_plan() == before


def _buffers(Npad, C, taps, B, Lin, N):
    g = _rng(81)
    wrec = vp3d.pack_weights(torch.from_numpy(g.standard_normal((N, taps * C)).astype(np.float32)), Npad, DEV)
    xrec = _cuda(R.pack(g.standard_normal((B * Lin, C)).astype(np.float32)).view(np.int16).reshape(-1))
    return wrec, xrec, _cuda(np.zeros(N, np.float32)), torch.empty((B * Lin, N), dtype=torch.float32, device=DEV)


@pytest.mark.parametrize("shape,force,piece", REFUSED_MM, ids=[p for _, _, p in REFUSED_MM])
def test_refused_forced_plans_mm(shape, force, piece):
    """An infeasible forced choice is an error that names its reason; nothing is launched, the last plan stays."""
    Npad, C, taps, dil, B, Lin = shape
    wrec, xrec, bias, out = _buffers(Npad, C, taps, B, Lin, Npad)
    launch("mm", make_layer(82, 16, 32, 1, 1, 1, 5, exact=True))          # a plan to be left alone
    _refused(lambda: vp3d.stream_mm(wrec, Npad, xrec, bias, out, Npad, None, B, Lin, C, taps, dil, Npad, force=force), piece)


def test_caps_no_forced_choice_can_reach():
    """Two of the planner's conditions hold for every choice that passes the others, so no forced choice is refused by
    them: the K-partials of a 4-wave pair, TAPS (CT / 16) RT 4 <= 80 KiB (at most 3 x 1 x 5 x 4 = 60 within RT <= 5), and
    the window kernel's LDS (a window of at most VP3D_WIN_MAX_NR = 512 rows is 128 KiB, the partials of TA 2 x RT 8
    are 128 KiB, both below 160).  Every NW = 4 row and every window row is accepted in test_every_instantiation."""
    assert max(t * (ct // 16) * rt * 4 for _, ct, rt, t, nw in [r for r in INSTANTIATIONS if r[0] == "conv"] if nw == 4) <= 80
    assert max(2 * 128 * 512, 8 * 2 * 8 * 1024) <= 160 * 1024


REFUSED_WIN = [
    ((48, 32, 3, 2, 23), (2, 1), "not a multiple of 16 TA"),
    ((32, 32, 3, 2, 23), (3, 1), "TA 3"),
    ((32, 32, 3, 2, 23), (1, 22), "exceeds Lout"),
    ((32, 32, 3, 2, 200), (1, 1), "at most 8 fit"),
    ((32, 32, 497, 2, 540), (1, 1), "staged rows"),        # RT 3: a window of 544 rows
]


@pytest.mark.parametrize("shape,force,piece", REFUSED_WIN, ids=[p for _, _, p in REFUSED_WIN])
def test_refused_forced_plans_win(shape, force, piece):
    Npad, C, taps, B, Lin = shape
    wrec, xrec, bias, out = _buffers(Npad, C, taps, B, Lin, Npad)
    launch("mm", make_layer(82, 16, 32, 1, 1, 1, 5, exact=True))
    _refused(lambda: vp3d.stream_win(wrec, Npad, xrec, bias, out, Npad, None, B, Lin, C, taps, Npad, force=force), piece)


@pytest.mark.parametrize("valu,force,piece", [(False, 39, "exceeds Lout"), (True, 1, "rows per workgroup"),
                                              (True, 77, "exceeds the 76 rows"), (False, -1, "negative")])
def test_refused_forced_plans_expand(valu, force, piece):
    g = _rng(83)
    B, Lin, Cin, taps, C = 2, 40, 34, 3, 32
    L = Layer(g.standard_normal((C, taps, Cin)).astype(np.float32), g.standard_normal((B, Lin, Cin)).astype(np.float32),
              np.zeros(C, np.float32))
    launch("mm", make_layer(82, 16, 32, 1, 1, 1, 5, exact=True))
    _refused(lambda: launch("evalu" if valu else "emfma", L, force), piece)


def test_refused_row_tiles_expand():
    g = _rng(84)
    L = Layer(g.standard_normal((32, 3, 34)).astype(np.float32), g.standard_normal((1, 103, 34)).astype(np.float32), np.zeros(32, np.float32))
    launch("mm", make_layer(82, 16, 32, 1, 1, 1, 5, exact=True))
    _refused(lambda: launch("emfma", L, 1), "at most 5 fit")       # 101 rows: 7 tiles


# ---- 5i: whole models off the beaten shape -----------------------------------------------------------------------------
@pytest.mark.parametrize("joints_out", [12, 17])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("dense", [False, True])
@pytest.mark.parametrize("channels", [96, 160])
def test_whole_model_off_the_beaten_shape(channels, dense, causal, joints_out):
    """TemporalModel at channel counts whose K loops have empty and unequal waves, against the float64 restated forward:
    inside the per-layer bounds of the random-data tests propagated through that forward (vp3d_stream_restated.forward)
    -- a worst-case bound that grows with every layer's sum of |W| and is far from sharp (profiles/vp3d_stream_unit.md
    has both figures) -- and inside the suite's whole-model tolerance, 2e-4 max |ref|."""
    fw = [3, 3, 3]
    sd = W.make_vp3d_state_dict(seed=3, joints_out=joints_out, filter_widths=fw, channels=channels, dense=dense)
    m = vp3d.TemporalModel(17, 2, joints_out, fw, causal=causal, channels=channels, dense=dense, prec=PREC_BF16X3)
    m.load_state_dict(sd)
    rf = m.receptive_field()
    assert rf == R.receptive_field(fw)
    worst_b = worst_t = 0.0
    for B in (1, 2):
        for frames in (rf, rf + 21):
            x = torch.randn(B, frames, 17, 2, generator=torch.Generator().manual_seed(B * 100 + frames))
            out = m(x.to(DEV)).cpu().numpy().astype(np.float64)
            ref, bound = R.forward(sd, x.numpy(), fw, causal=causal, dense=dense, with_bound=True)
            assert out.shape == ref.shape == (B, frames - rf + 1, joints_out, 3)
            err = np.abs(out - ref)
            worst_b = max(worst_b, float((err / bound).max()))
            worst_t = max(worst_t, float(err.max() / (2e-4 * max(1.0, np.abs(ref).max()))))
            fam = vp3d.last_plan()[0]
            assert fam in (CONV, MM)        # the shrink layer ran on the streaming path
    print(f"RATIO model C={channels} dense={dense} propagated {worst_b:.2e} suite-tolerance {worst_t:.4f}")
    assert worst_b <= 1.0 and worst_t <= 1.0
