"""Restatement of the direct 3x3 -> 32 convolution of the DPT heads (csrc/conv_direct.hip, skimi_conv3x3_n32 and
skimi_conv3x3_n32_strided in include/skimi.h), for test_conv_direct_cpu.py and test_conv_direct_gpu.py.  It knows nothing
about tiles, windows or swizzles:

  * `reference`: the documented operation in float64 as explicit index arithmetic (window origin (y - 1, x - 1), zero
    outside the image, a frame reads only itself), pinned on the CPU against float64 F.conv2d(padding=1);
  * `pack_restated`: the documented layout of the packed weight, [Cin/32][hi | lo][tap = ky * 3 + kx][cout][cin % 32];
  * operand builders whose contraction is exact in fp32 whatever the order of the MFMA's sums (`exact_operands`), and
    the plane split hi = bf16(x), lo = bf16(x - hi) the kernel's operands are made by (`split_hi_lo`);
  * `guarded`: a tensor inside a NaN-filled buffer, so that a read from outside the planes poisons the result and a
    store outside the output shows.

Why the exact families are exact.  The kernel computes sum (a_lo w_hi + a_hi w_lo + a_hi w_hi) and drops a_lo w_lo, so one
operand of each family has lo == 0 everywhere.  All values are integers times one power of two q, every bf16 half is
such an integer too, and sum (|a_hi| + |a_lo|) (|w_hi| + |w_lo|) / q stays below 2^24 at C = 256 (asserted on the CPU):
every product and every partial sum of any subset of the terms is an integer multiple of q below 2^24 q, which fp32
holds exactly.  The bias is a small integer, and the sum with it stays below 2^24 q as well."""
import torch

SHAPES = [(1, 1, 1, 32), (2, 16, 16, 32), (3, 16, 16, 64), (3, 17, 15, 64), (1, 33, 18, 96), (2, 5, 40, 128),
          (1, 48, 32, 256)]   # (F, H, W, C): what each is there to catch is in test_conv_direct_gpu.py
FAMILIES = ("ints_small", "ints_a_lo", "ints_w_lo")
W_SHIFT = 8   # ints_w_lo: W = integers * 2^-W_SHIFT


def gen(seed):
    return torch.Generator().manual_seed(seed)


def reference(x, w, bias=None, relu=False):
    """x [F, H, W, C], w [32, C, 3, 3], bias [32] or None (float64) -> [F, H, W, 32] float64, channels-last"""
    F_, H, W_, C = x.shape
    Co = w.shape[0]
    assert w.shape == (Co, C, 3, 3) and x.dtype == torch.float64 and w.dtype == torch.float64
    flat = x.reshape(-1, C)
    m = torch.arange(F_ * H * W_)
    f, oy, ox = m // (H * W_), (m // W_) % H, m % W_
    out = torch.zeros(F_ * H * W_, Co, dtype=torch.float64)
    for ky in range(3):
        for kx in range(3):
            iy, ix = oy - 1 + ky, ox - 1 + kx
            inside = (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W_)
            src = (f * H + iy.clamp(0, H - 1)) * W_ + ix.clamp(0, W_ - 1)
            a = torch.where(inside[:, None], flat[src], torch.zeros((), dtype=torch.float64))
            out += a @ w[:, :, ky, kx].T
    if bias is not None:
        out = out + bias.double()
    if relu:
        out = out.clamp_min(0.0)
    return out.view(F_, H, W_, Co)


def split_hi_lo(x):
    """fp32 -> (hi, lo) bf16: hi = bf16(x), lo = bf16(x - float(hi)), round to nearest even"""
    x = x.float()
    hi = x.to(torch.bfloat16)
    return hi, (x - hi.float()).to(torch.bfloat16)


def pack_restated(w):
    """w [32, C, 3, 3] fp32 -> bf16 [C/32, 2, 9, 32, 32] = [slice][hi | lo][tap = ky * 3 + kx][cout][cin % 32]"""
    Co, C, kh, kw = w.shape
    assert (Co, kh, kw) == (32, 3, 3) and C % 32 == 0 and w.dtype == torch.float32
    planes = torch.stack(split_hi_lo(w))                                  # [plane, cout, cin, ky, kx]
    named = planes.unflatten(2, (C // 32, 32)).flatten(4, 5)               # [plane, cout, slice, cin % 32, tap]
    return named.movedim((2, 0, 4, 1, 3), (0, 1, 2, 3, 4)).contiguous()   # -> [slice, plane, tap, cout, cin % 32]


def exact_operands(family, shape, seed, bias=True):
    """(x [F, H, W, C], w [32, C, 3, 3], bias [32] or None) float64, exactly representable in fp32 and such that the
    kernel's contraction is exact (module docstring)"""
    F_, H, W_, C = shape
    g = gen(seed)

    def ints(shp, lim):
        return torch.randint(-lim, lim + 1, shp, generator=g).double()

    if family == "ints_small":      # lo == 0 everywhere: the pure index path
        x, w = ints((F_, H, W_, C), 3), ints((32, C, 3, 3), 2)
    elif family == "ints_a_lo":     # wide A, narrow W: the a_lo . w_hi term
        x, w = ints((F_, H, W_, C), 2047), ints((32, C, 3, 3), 2)
    elif family == "ints_w_lo":     # wide W, narrow A: the a_hi . w_lo term
        x, w = ints((F_, H, W_, C), 3), ints((32, C, 3, 3), 2047) * 2.0 ** -W_SHIFT
    else:
        raise ValueError(family)
    return x, w, (ints((32,), 8) if bias else None)


def exact_unit(family):
    """the power of two q all values of the family are integer multiples of"""
    return 2.0 ** -W_SHIFT if family == "ints_w_lo" else 1.0


def interleave(hi, lo):
    """planes [F, H, W, C] -> the DPT heads' pixel records [F, H, W, hi C | lo C]"""
    return torch.cat([hi, lo], dim=-1).contiguous()


def guarded(t, guard, device=None):
    """t [..., E] (E elements per pixel) inside a larger NaN-filled buffer of t's dtype, `guard` pixels in front of the
    first frame and behind the last -> (the view holding t, the whole flat buffer)"""
    E = t.shape[-1]
    npix = t.numel() // E
    buf = torch.full(((npix + 2 * guard) * E,), float("nan"), dtype=t.dtype, device=device or t.device)
    view = buf[guard * E:(guard + npix) * E].view(t.shape)
    view.copy_(t)
    return view, buf


def first_wrong(got, want):
    """(count, (f, y, x, co) of the first) of the elements of got [F, H, W, 32] that differ from want (NaN differs)"""
    bad = ~(got == want)
    if not bad.any():
        return 0, None
    return int(bad.sum()), tuple(int(i) for i in bad.nonzero()[0])
