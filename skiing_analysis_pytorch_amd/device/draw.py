"""Drawing into uint8 frame clips (csrc/draw.hip; C-ABI: skimi_draw_shapes_u8): the rasteriser's wrapper and the builders
of its shape records; the reference's drawing functions (the package's draw.py, bev.draw_points) are built on these; rules:
include/skimi.h, DESIGN §2 "Drawing".

draw_shapes is the one launch.  The builders are plain torch ops on whatever device their inputs are on (so they run in
CPU tests) and never read back: a joint that is NaN, or below a score threshold, becomes a record of kind 0, which the
kernel draws as nothing.  A list is int32 [..., P, 8] under the frames' leading axes ([P, 8]: shared by every frame); lists
are joined in drawing order with cat_shapes.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import font5x7
from .._args import frame_clip, frame_out, on_device
from .._lib import check, current_stream, lib, ptr

DRAW_MAX_SHAPES = 1024
DRAW_NONE, DRAW_DISC, DRAW_RING, DRAW_CAPSULE, DRAW_GLYPH = 0, 1, 2, 3, 4
GLYPH_ADVANCE = 6      # pixels per character at scale 1: the 5-pixel cell and one of space
GLYPH_HEIGHT = 7
_LIMIT = float(1 << 24)   # builders clamp positions here, inside int32; the kernel saturates to +-2^20 itself

font_5x7 = font5x7.font_5x7
_fonts = {}


def _default_font(dev):
    """the project's font on dev, uploaded once per device"""
    if dev not in _fonts:
        _fonts[dev] = torch.from_numpy(font_5x7()).to(dev)
    return _fonts[dev]


def draw_shapes(frames: torch.Tensor, shapes: torch.Tensor, font=None, out=None, inplace: bool = False) -> torch.Tensor:
    """Draw an ordered list of shapes into every frame of a clip in one launch: frames uint8 [F, H, W, ch] or [C, F, H, W, ch]
    (ch 1, 3 or 4), shapes int32 [P, 8] (every frame draws the same list), [F, P, 8] or, for five-axis frames, [C, F, P, 8],
    P <= DRAW_MAX_SHAPES, both on the device -> the drawn frames.  Records (kind, x0, y0, x1, y1, r, colour, opacity) and the
    rules are include/skimi.h's; later records paint over earlier ones.  font: uint8 [96, 7] on the device (default: the
    project's font_5x7).  The input is not modified unless inplace=True (then it must be contiguous, and it is what is
    returned); out: a preallocated result.  Nothing is read back."""
    fr, five = frame_clip("draw_shapes", frames)
    on_device("draw_shapes", shapes=shapes, font=font)
    if shapes.dtype != torch.int32 or shapes.dim() not in (2, 3, 4) or shapes.shape[-1] != 8:
        raise ValueError(f"draw_shapes: shapes must be int32 [P, 8], [F, P, 8] or [C, F, P, 8], got {shapes.dtype} {list(shapes.shape)}")
    C, F, H, W, ch = (int(s) for s in fr.shape)
    P = int(shapes.shape[-2])
    lead = {2: (), 3: (F,), 4: (C, F)}[shapes.dim()]
    if tuple(shapes.shape[:-2]) != lead or (shapes.dim() == 4 and not five):
        raise ValueError(f"draw_shapes: shapes {list(shapes.shape)} do not match frames {list(frames.shape)}")
    if P > DRAW_MAX_SHAPES:
        raise ValueError(f"draw_shapes: {P} shapes in a list, at most {DRAW_MAX_SHAPES}")
    if font is None:
        font = _default_font(fr.device)
    elif font.dtype != torch.uint8 or tuple(font.shape) != (96, 7):
        raise ValueError(f"draw_shapes: font must be uint8 [96, 7], got {font.dtype} {list(font.shape)}")
    if inplace:
        if out is not None or not frames.is_contiguous():
            raise ValueError("draw_shapes: inplace=True needs contiguous frames and no out")
        res = frames
    else:
        res = frame_out("draw_shapes", fr, five, W, H, out)
    if C * F == 0:
        return res
    sh, fo = shapes.to(fr.device).contiguous(), font.to(fr.device).contiguous()
    check(lib().skimi_draw_shapes_u8(ptr(fr), ptr(res), ptr(sh), sh.dim(), ptr(fo), C, F, H, W, ch, P, current_stream()),
          "skimi_draw_shapes_u8")
    return res


# ---- builders ------------------------------------------------------------------------------------------------------------
def pack_colour(colour) -> int:
    """(c0, c1, c2) or one number -> 0x00c2c1c0: channel i of the frame gets element i (a 1-channel frame the first)"""
    c = [int(colour)] * 3 if np.isscalar(colour) else [int(v) for v in colour][:3]
    if len(c) != 3 or any(v < 0 or v > 255 for v in c):
        raise ValueError(f"colour must be one or three numbers in 0 .. 255, got {colour!r}")
    return c[0] | (c[1] << 8) | (c[2] << 16)


def _positions(xy, subpixel):
    """[..., 2] pixels -> (int64 [..., 2] in 1/16 pixel, bool [...]: both coordinates finite).  Whole pixels, rounded half to
    even as the reference's int(round(x)), unless subpixel (then 16 x is rounded)."""
    x = torch.as_tensor(xy).to(torch.float64)
    if x.dim() < 1 or x.shape[-1] != 2:
        raise ValueError(f"positions must be [..., 2], got {list(x.shape)}")
    fin = torch.isfinite(x).all(dim=-1)
    x = torch.where(fin[..., None], x, torch.zeros_like(x))
    q = torch.round(x * 16.0) if subpixel else torch.round(x) * 16.0
    return q.clamp(-_LIMIT, _LIMIT).to(torch.int64), fin


def _sixteenths(v, like, scale=16.0):
    """a length in pixels, a number or a tensor broadcastable to like's shape -> int64 of like's shape, in 1/16 pixel"""
    t = torch.as_tensor(v, dtype=torch.float64, device=like.device)
    return torch.round(t * scale).clamp(-_LIMIT, _LIMIT).to(torch.int64).expand(like.shape)


def _records(kind, x0, y0, x1, y1, r, colour, opacity, ok):
    """the eight words side by side -> int32 [..., 8]; a record that is not ok is all zero (kind 0)"""
    full = lambda v: torch.as_tensor(v, dtype=torch.int64, device=x0.device).expand(x0.shape)   # noqa: E731
    rec = torch.stack([full(kind), x0, y0, full(x1), full(y1), full(r), full(colour), full(int(opacity))], dim=-1)
    return torch.where(ok[..., None], rec, torch.zeros_like(rec)).to(torch.int32)


def _valid(fin, valid):
    return fin if valid is None else fin & torch.as_tensor(valid, device=fin.device).to(torch.bool)


def disc_shapes(xy, radius, colour, thickness=-1, opacity=256, valid=None, subpixel=False) -> torch.Tensor:
    """cv2.circle as records: xy [..., n, 2] float pixels -> int32 [..., n, 8].  thickness < 0: a filled disc of `radius` pixels;
    else a ring whose line is `thickness` pixels wide (half thickness 8 thickness sixteenths).  radius: a number or [..., n].
    A non-finite position or valid == False gives kind 0."""
    p, fin = _positions(xy, subpixel)
    x0, y0 = p[..., 0], p[..., 1]
    r = _sixteenths(radius, x0)
    zero = torch.zeros_like(x0)
    if thickness is None or thickness < 0:
        return _records(DRAW_DISC, x0, y0, zero, zero, r, pack_colour(colour), opacity, _valid(fin, valid))
    return _records(DRAW_RING, x0, y0, _sixteenths(thickness, x0, 8.0), zero, r, pack_colour(colour), opacity, _valid(fin, valid))


def segment_shapes(xy0, xy1, colour, thickness=1, opacity=256, valid=None, subpixel=False) -> torch.Tensor:
    """cv2.line as records: xy0, xy1 [..., n, 2] -> int32 [..., n, 8], capsules of half width 8 thickness sixteenths.  A
    segment with a non-finite end, or valid == False, gives kind 0."""
    a, fa = _positions(xy0, subpixel)
    b, fb = _positions(xy1, subpixel)
    if a.shape != b.shape:
        raise ValueError(f"segment_shapes: ends must have one shape, got {list(a.shape)}, {list(b.shape)}")
    return _records(DRAW_CAPSULE, a[..., 0], a[..., 1], b[..., 0], b[..., 1], _sixteenths(thickness, a[..., 0], 8.0), pack_colour(colour),
                    opacity, _valid(fa & fb, valid))


def polyline_shapes(xy, colour, thickness=1, closed=False, opacity=256, subpixel=False) -> torch.Tensor:
    """cv2.polylines as records: xy [..., n, 2] -> int32 [..., n - 1, 8] (closed: [..., n, 8], the last joins the first)."""
    x = torch.as_tensor(xy)
    nxt = torch.roll(x, -1, dims=-2)
    if not closed:
        x, nxt = x[..., :-1, :], nxt[..., :-1, :]
    return segment_shapes(x, nxt, colour, thickness, opacity, None, subpixel)


def glyph_shapes(codes, left, top, scale, colour, opacity=256, valid=None) -> torch.Tensor:
    """One glyph record per entry: codes [..., n] character codes (outside 0x20 .. 0x7F: 0x7F, the filled box), left, top
    [..., n] the cell's top-left pixel (whole pixels) -> int32 [..., n, 8].  scale: an integer >= 1."""
    scale = int(scale)
    if scale < 1:
        raise ValueError(f"glyph scale must be an integer >= 1, got {scale}")
    left = torch.as_tensor(left)
    c = torch.as_tensor(codes, device=left.device).to(torch.int64)
    c = torch.where((c >= font5x7.FIRST) & (c <= font5x7.LAST), c, torch.full_like(c, font5x7.LAST))
    x0 = left.to(torch.int64) * 16
    c, x0 = torch.broadcast_tensors(c, x0)
    y0 = (torch.as_tensor(top, device=left.device).to(torch.int64) * 16).expand(x0.shape)
    ok = torch.ones_like(x0, dtype=torch.bool) if valid is None else torch.as_tensor(valid, device=left.device).to(torch.bool).expand(x0.shape)
    return _records(DRAW_GLYPH, x0, y0, c, torch.zeros_like(x0), scale, pack_colour(colour), opacity, ok)


def string_codes(strings, width=None) -> np.ndarray:
    """host strings -> int64 [len(strings), width] character codes, -1 behind a string's end (width: the longest's length)"""
    strings = [str(s) for s in strings]
    width = max([len(s) for s in strings], default=0) if width is None else int(width)
    codes = np.full((len(strings), width), -1, dtype=np.int64)
    for i, s in enumerate(strings):
        codes[i, :len(s)] = [ord(ch) for ch in s[:width]]
    return codes


def text_shapes(strings, anchor_xy, scale, colour, opacity=256, valid=None, subpixel=False) -> torch.Tensor:
    """cv2.putText as records: strings, a host list of S strings (or one string), anchor_xy [..., S, 2] float pixels (the text's
    BOTTOM-LEFT corner, cv2's org, rounded to whole pixels) -> int32 [..., total characters, 8], string after string, one
    glyph per character advancing 6 scale pixels; the bottom row of the 7 scale cell is the anchor's row.  The strings are
    host data, the anchors may be device data: nothing is read back.  A non-finite anchor or valid == False ([..., S]) gives
    kind 0 for the whole string."""
    if isinstance(strings, str):
        strings = [strings]
    scale = int(scale)
    p, fin = _positions(anchor_xy, False)
    if p.shape[-2] != len(strings):
        raise ValueError(f"text_shapes: {len(strings)} strings need anchors [..., {len(strings)}, 2], got {list(p.shape)}")
    ok = _valid(fin, valid)
    dev = p.device
    which = torch.tensor([i for i, s in enumerate(strings) for _ in s], dtype=torch.int64, device=dev)
    step = torch.tensor([k for s in strings for k in range(len(s))], dtype=torch.int64, device=dev)
    codes = torch.tensor([ord(ch) for s in strings for ch in s], dtype=torch.int64, device=dev)
    px = torch.div(p, 16, rounding_mode="floor")   # whole pixels
    left = px[..., 0].index_select(-1, which) + step * (GLYPH_ADVANCE * scale)
    top = px[..., 1].index_select(-1, which) - (GLYPH_HEIGHT * scale - 1)
    return glyph_shapes(codes, left, top, scale, colour, opacity, ok.index_select(-1, which))


def number_shapes(numbers, anchor_xy, digits, scale, colour, opacity=256, valid=None) -> torch.Tensor:
    """str(n) of DEVICE integers 0 <= n < 10^digits as records, left-aligned at anchor_xy (text_shapes' bottom-left corner):
    numbers [..., n], anchor_xy [..., n, 2] -> int32 [..., n * digits, 8]; the places a shorter number does not use are kind
    0.  For labels that depend on device data (the running index of the joints that pass a score filter)."""
    scale, digits = int(scale), int(digits)
    p, fin = _positions(anchor_xy, False)
    ok = _valid(fin, valid)
    n = torch.as_tensor(numbers, device=p.device).to(torch.int64)
    length = torch.ones_like(n)
    for k in range(1, digits):
        length = length + (n >= 10 ** k).to(torch.int64)
    place = torch.arange(digits, dtype=torch.int64, device=p.device)            # from the left
    power = (length[..., None] - 1 - place).clamp(min=0)
    digit = torch.div(n[..., None], 10 ** power, rounding_mode="floor") % 10
    used = (place < length[..., None]) & ok[..., None] & (n[..., None] >= 0)
    px = torch.div(p, 16, rounding_mode="floor")
    left = px[..., 0, None] + place * (GLYPH_ADVANCE * scale)
    top = (px[..., 1, None] - (GLYPH_HEIGHT * scale - 1)).expand(left.shape)
    rec = glyph_shapes(digit + ord("0"), left, top, scale, colour, opacity, used)
    return rec.reshape(*rec.shape[:-3], rec.shape[-3] * digits, 8)


def cat_shapes(*lists) -> torch.Tensor:
    """lists in drawing order -> one list [..., P, 8]; a list with fewer leading axes is repeated under the others' axes"""
    lists = [x for x in lists if x is not None]
    lead = torch.broadcast_shapes(*[tuple(x.shape[:-2]) for x in lists])
    return torch.cat([x.expand(*lead, *x.shape[-2:]) for x in lists], dim=-2).contiguous()
