"""CPU: the restatement test_conv_direct_gpu.py compares the direct 3x3 conv with (conv_direct_restated.py) is pinned
against torch, and the exactness preconditions of its operand families hold.  No kernel runs here."""
import pytest
import torch
import torch.nn.functional as F

import conv_direct_restated as R


def _conv2d(x, w, bias=None, relu=False):
    y = F.conv2d(x.permute(0, 3, 1, 2), w, bias, padding=1)
    return (F.relu(y) if relu else y).permute(0, 2, 3, 1)


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_reference_matches_conv2d(shape):
    g = R.gen(7 + R.SHAPES.index(shape))
    x = torch.randn(shape, generator=g, dtype=torch.float64)
    w = torch.randn(32, shape[3], 3, 3, generator=g, dtype=torch.float64)
    b = torch.randn(32, generator=g, dtype=torch.float64)
    for bias, relu in ((None, False), (b, False), (b, True)):
        got, want = R.reference(x, w, bias, relu), _conv2d(x, w, bias, relu)
        assert got.shape == want.shape == (*shape[:3], 32)
        assert torch.allclose(got, want, rtol=1e-12, atol=1e-12), (shape, float((got - want).abs().max()))


def test_reference_seams_and_borders():
    """what a comparison on random data shows only weakly: a frame reads only itself, and a tap outside the image
    contributes exactly zero.  With all-ones weights an output is the plain sum of the pixels under the window."""
    x = torch.zeros(3, 2, 2, 32, dtype=torch.float64)
    x[0], x[1], x[2] = 1.0, 100.0, 10000.0
    w = torch.zeros(32, 32, 3, 3, dtype=torch.float64)
    w[:, 0] = 1.0                                    # channel 0 only: every output is the count of inside pixels
    out = R.reference(x, w)
    for f, v in enumerate((1.0, 100.0, 10000.0)):   # a 2 x 2 frame: all four pixels lie under every window
        assert torch.equal(out[f], torch.full((2, 2, 32), 4 * v, dtype=torch.float64))
    # one tap, window origin (y - 1, x - 1): tap (ky, kx) = (0, 2) reads (y - 1, x + 1)
    x = torch.randn(1, 4, 5, 32, generator=R.gen(1), dtype=torch.float64)
    w = torch.zeros(32, 32, 3, 3, dtype=torch.float64)
    w[3, 5, 0, 2] = 1.0
    out = R.reference(x, w)
    want = torch.zeros(4, 5, dtype=torch.float64)
    want[1:, :4] = x[0, :3, 1:, 5]
    assert torch.equal(out[0, :, :, 3], want) and not out[..., :3].any() and not out[..., 4:].any()


@pytest.mark.parametrize("C", [32, 96, 256])
def test_pack_restated_against_permutation(C):
    w = torch.randn(32, C, 3, 3, generator=R.gen(C))
    w[::3, ::5] = w[::3, ::5].to(torch.bfloat16).float()   # lo == 0
    w[1, ::7] = 0.0
    got = R.pack_restated(w)
    assert got.shape == (C // 32, 2, 9, 32, 32) and got.dtype == torch.bfloat16 and got.is_contiguous()
    hi = w.to(torch.bfloat16)
    lo = (w - hi.float()).to(torch.bfloat16)
    assert (lo.float() != 0).any() and (lo[::3, ::5].float() == 0).all()
    want = torch.stack([p.reshape(32, C // 32, 32, 9).permute(1, 3, 0, 2) for p in (hi, lo)], dim=1)
    assert torch.equal(got.view(torch.int16), want.contiguous().view(torch.int16))
    # and the documented formula, element by element on a sample
    flat = got.reshape(-1).float()
    for cs, p, tap, co, c32 in ((0, 0, 0, 0, 0), (C // 32 - 1, 1, 8, 31, 31), (0, 1, 5, 7, 13), (C // 64, 0, 3, 30, 1)):
        src = (hi, lo)[p][co, cs * 32 + c32, tap // 3, tap % 3]
        assert flat[(((cs * 2 + p) * 9 + tap) * 32 + co) * 32 + c32] == float(src)


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("C", [32, 256])
def test_exact_families_are_exact_in_fp32(family, C):
    """the three properties that make every product and every partial sum of the kernel exact, whatever its order"""
    x, w, b = R.exact_operands(family, (1, 48, 32, C), seed=5)
    q = R.exact_unit(family)
    wide = {"ints_small": None, "ints_a_lo": x, "ints_w_lo": w}[family]
    for t in (x, w):
        assert torch.equal(t.float().double(), t)                       # exactly an fp32 value
        hi, lo = R.split_hi_lo(t)
        assert torch.equal(hi.double() + lo.double(), t), "float(hi) + float(lo) == x"
        for h in (hi, lo):
            assert torch.equal((h.double() / q).round() * q, h.double())    # a multiple of the unit
        if t is wide:
            assert (lo.float() != 0).double().mean() >= 0.5, "at least half of the lo halves must be nonzero"
        else:
            assert not lo.float().any(), "never two wide operands: the kernel drops lo * lo"
    # sum of |a| |w| over the window, in units of q, at the bias's worst
    mag = R.reference(x.abs(), w.abs()) / q
    assert float(mag.max()) + 8 / q < 2.0 ** 24
    ah, al = R.split_hi_lo(x)
    wh, wl = R.split_hi_lo(w)
    mag2 = R.reference(ah.double().abs() + al.double().abs(), wh.double().abs() + wl.double().abs()) / q
    assert float(mag2.max()) + 8 / q < 2.0 ** 24
    # and the worst case of the value ranges, not only of this draw
    amax, wmax = {"ints_small": (3, 2), "ints_a_lo": (2048 + 8, 2), "ints_w_lo": (3, 2048 + 8)}[family]
    assert amax * wmax * 9 * 256 + 8 / q < 2.0 ** 24
    assert b is not None and torch.equal(b, b.round()) and float(b.abs().max()) <= 8


def test_guarded_layout():
    t = torch.arange(2 * 3 * 4 * 8, dtype=torch.float32).view(2, 3, 4, 8).to(torch.bfloat16)
    view, buf = R.guarded(t, 5)
    assert buf.numel() == (24 + 10) * 8 and view.data_ptr() == buf.data_ptr() + 5 * 8 * 2
    assert torch.equal(view, t) and torch.isnan(buf[:40]).all() and torch.isnan(buf[-40:]).all()
    rec = R.interleave(t, -t)
    assert rec.shape == (2, 3, 4, 16) and torch.equal(rec[..., :8], t) and torch.equal(rec[..., 8:], -t)
    assert R.first_wrong(view, t) == (0, None)
    view[1, 2, 0, 3] = float("nan")
    assert R.first_wrong(view, t) == (1, (1, 2, 0, 3))
