"""NumPy restatement of the drawing rules (include/skimi.h, the drawing block; DESIGN §2 "Drawing"), written from the rules
and not from the kernel: no tiles, no lists, one loop over the shapes in list order, each over its own bounding box, all
in int64.  The device result must equal it byte for byte."""
import math

import numpy as np

MAX_SHAPES = 1024
NONE, DISC, RING, CAPSULE, GLYPH = 0, 1, 2, 3, 4
SAT = 1 << 20


def sat(v):
    return max(-SAT, min(SAT, int(v)))


def isqrt(n):
    """exact floor square root of an int64 array"""
    return np.vectorize(math.isqrt, otypes=[np.int64])(n) if n.size else n.astype(np.int64)


def coverage(rec, u, v, font):
    """cov 0 .. 16 of the pixels (u, v) (int64 arrays of one shape) under one record; None: the record draws nothing"""
    kind, x0, y0, x1, y1, r = (int(w) for w in rec[:6])
    if kind < DISC or kind > GLYPH:
        return None
    x0, y0, r = sat(x0), sat(y0), sat(r)
    if kind == GLYPH:
        s = max(r, 1)
        code = x1 if 0x20 <= x1 <= 0x7F else 0x7F
        left, top = x0 >> 4, y0 >> 4            # floor
        cx, cy = u - left, v - top
        inside = (cx >= 0) & (cy >= 0) & (cx < 5 * s) & (cy < 7 * s)
        rows = font[code - 0x20].astype(np.int64)[np.clip(cy // s, 0, 6)]
        return np.where(inside & (((rows >> np.clip(cx // s, 0, 4)) & 1) == 1), 16, 0)
    x1, y1 = sat(x1), sat(y1)
    px, py = 16 * u - x0, 16 * v - y0
    da = isqrt(px * px + py * py)
    if kind == DISC:
        return np.clip(r + 8 - da, 0, 16)
    if kind == RING:
        return np.clip(x1 + 8 - np.abs(da - r), 0, 16)
    ex, ey = x1 - x0, y1 - y0
    L2 = ex * ex + ey * ey
    if L2 == 0:
        return np.clip(r + 8 - da, 0, 16)
    t = px * ex + py * ey
    qx, qy = px - ex, py - ey
    db = isqrt(qx * qx + qy * qy)
    dl = np.abs(px * ey - py * ex) // math.isqrt(L2)
    d = np.where(t <= 0, da, np.where(t >= L2, db, dl))
    return np.clip(r + 8 - d, 0, 16)


def bounding_box(rec, H, W):
    """pixel rows and columns [v0, v1) x [u0, u1) of the frame outside which the record's coverage is 0: its extent grown by the
    radius plus one pixel"""
    kind, x0, y0, x1, y1, r = (int(w) for w in rec[:6])
    x0, y0, r = sat(x0), sat(y0), sat(r)
    if kind == GLYPH:
        s = max(r, 1)
        lo_x, lo_y = (x0 >> 4) * 16, (y0 >> 4) * 16
        hi_x, hi_y, g = lo_x + 16 * 5 * s, lo_y + 16 * 7 * s, 16
    else:
        x1, y1 = sat(x1), sat(y1)
        g = r + 16 + (x1 if kind == RING else 0)
        if kind == CAPSULE:
            lo_x, hi_x, lo_y, hi_y = min(x0, x1), max(x0, x1), min(y0, y1), max(y0, y1)
        else:
            lo_x = hi_x = x0
            lo_y = hi_y = y0
    u0, u1 = max((lo_x - g) // 16, 0), min((hi_x + g) // 16 + 2, W)
    v0, v1 = max((lo_y - g) // 16, 0), min((hi_y + g) // 16 + 2, H)
    return v0, v1, u0, u1


def draw_frame(frame, shapes, font):
    """frame uint8 [H, W, ch], shapes int [P, 8], font uint8 [96, 7] -> the drawn frame (a new array)"""
    H, W, ch = frame.shape
    out = frame.astype(np.int64)
    for rec in np.asarray(shapes, dtype=np.int64).reshape(-1, 8):
        opacity = max(0, min(256, int(rec[7])))
        if opacity == 0 or not (DISC <= int(rec[0]) <= GLYPH):
            continue
        v0, v1, u0, u1 = bounding_box(rec, H, W)
        if v0 >= v1 or u0 >= u1:
            continue
        v, u = np.meshgrid(np.arange(v0, v1, dtype=np.int64), np.arange(u0, u1, dtype=np.int64), indexing="ij")
        a = coverage(rec, u, v, font) * opacity
        for c in range(min(ch, 3)):
            col = (int(rec[6]) >> (8 * c)) & 255
            cur = out[v0:v1, u0:u1, c]
            out[v0:v1, u0:u1, c] = np.where(a == 0, cur, (cur * (4096 - a) + col * a + 2048) >> 12)
    return out.astype(np.uint8)


def draw_clip(frames, shapes, font):
    """frames uint8 [F, H, W, ch] or [C, F, H, W, ch]; shapes [P, 8], [F, P, 8] or [C, F, P, 8] -> the drawn clip"""
    frames, shapes = np.asarray(frames), np.asarray(shapes)
    five = frames.ndim == 5
    fr = frames if five else frames[None]
    C, F = fr.shape[:2]
    out = np.empty_like(fr)
    for c in range(C):
        for f in range(F):
            lst = shapes if shapes.ndim == 2 else shapes[f] if shapes.ndim == 3 else shapes[c, f]
            out[c, f] = draw_frame(fr[c, f], lst, font)
    return out if five else out[0]


def reprojection_stats(kpt, proj):
    """vggt/reproject.py: RMSE, mean, median, max of |proj - kpt| per frame, NaN joints skipped: [..., J, 2] -> [..., 4]"""
    err = np.linalg.norm(np.asarray(proj, float) - np.asarray(kpt, float), axis=-1)
    return np.stack([np.sqrt(np.nanmean(err ** 2, axis=-1)), np.nanmean(err, axis=-1), np.nanmedian(err, axis=-1), np.nanmax(err, axis=-1)],
                    axis=-1)
