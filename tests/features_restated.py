"""NumPy restatement of the image-feature rules (include/skimi.h "ORB-style image features", DESIGN §2 "Image features"),
written from the rules and not from csrc/features.hip: the same integer expressions, evaluated on whole arrays in int64.

    orb_features(frame, max_features, levels, threshold, roi) -> dict of the outputs of geometry.orb_features for one frame
    match_hamming(d1, d2, ...)                                -> (pairs, dist, count) for one pair of descriptor sets
"""
import math

import numpy as np

MAX_LEVELS, BORDER = 8, 16
PATTERN_SEED = 0x534B494D494F5242
MASK64 = (1 << 64) - 1
RING = [(0, -3), (1, -3), (2, -2), (3, -1), (3, 0), (3, 1), (2, 2), (1, 3), (0, 3), (-1, 3), (-2, 2), (-3, 1), (-3, 0), (-3, -1),
        (-2, -2), (-1, -3)]
COS = [int(round(2 ** 14 * math.cos(2 * math.pi * k / 32))) for k in range(32)]
SIN = [int(round(2 ** 14 * math.sin(2 * math.pi * k / 32))) for k in range(32)]


# ---- the pattern -----------------------------------------------------------------------------------------------------
def splitmix64(s):
    s = (s + 0x9E3779B97F4A7C15) & MASK64
    z = s
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return s, z ^ (z >> 31)


def base_pattern():
    s, out, seen = PATTERN_SEED, [], set()
    while len(out) < 256:
        v = []
        for _ in range(4):
            s, z = splitmix64(s)
            v.append(int(z % 27) - 13)
        ax, ay, bx, by = v
        if ax * ax + ay * ay > 169 or bx * bx + by * by > 169 or (ax, ay) == (bx, by) or tuple(v) in seen:
            continue
        seen.add(tuple(v))
        out.append(v)
    return np.array(out, dtype=np.int64)


def rotated_patterns():
    """[32, 256, 4] int64"""
    base = base_pattern()
    tab = np.zeros((32, 256, 4), dtype=np.int64)
    for k in range(32):
        c, s = COS[k], SIN[k]
        for h in (0, 2):
            x, y = base[:, h], base[:, h + 1]
            tab[k, :, h] = (x * c - y * s + 8192) >> 14
            tab[k, :, h + 1] = (x * s + y * c + 8192) >> 14
    return tab


_PATTERNS = None


def patterns():
    global _PATTERNS
    if _PATTERNS is None:
        _PATTERNS = rotated_patterns()
    return _PATTERNS


# ---- the pyramid -----------------------------------------------------------------------------------------------------
def gray(frame):
    f = np.asarray(frame).astype(np.int64)
    if f.ndim == 2:
        return f
    if f.shape[2] == 1:
        return f[:, :, 0]
    return (3735 * f[:, :, 0] + 19235 * f[:, :, 1] + 9798 * f[:, :, 2] + 16384) >> 15


def level_size(n, l):
    return (2 * n * 5 ** l + 6 ** l) // (2 * 6 ** l)


def _axis(n_src, n_dst):
    x = np.arange(n_dst, dtype=np.int64)
    n, den = (2 * x + 1) * n_src - n_dst, 2 * n_dst
    x0 = n // den
    a = ((n - x0 * den) * 256) // den
    return np.clip(x0, 0, n_src - 1), np.clip(x0 + 1, 0, n_src - 1), a


def shrink(src, w, h):
    x0, x1, ax = _axis(src.shape[1], w)
    y0, y1, ay = _axis(src.shape[0], h)
    ax, ay = ax[None, :], ay[:, None]
    top = (256 - ax) * src[y0][:, x0] + ax * src[y0][:, x1]
    bot = (256 - ax) * src[y1][:, x0] + ax * src[y1][:, x1]
    return ((256 - ay) * top + ay * bot + (1 << 15)) >> 16


def blur5(img):
    p = np.pad(img, 2, mode="edge")
    k = (1, 4, 6, 4, 1)
    H, W = img.shape
    rows = sum(k[i] * p[:, i:i + W] for i in range(5))
    v = sum(k[i] * rows[i:i + H, :] for i in range(5))
    return (v + 128) >> 8


def pyramid(frame, levels):
    g = [gray(frame)]
    H, W = g[0].shape
    for l in range(1, levels):
        g.append(shrink(g[-1], level_size(W, l), level_size(H, l)))
    return g, [blur5(a) for a in g]


# ---- FAST ------------------------------------------------------------------------------------------------------------
def fast_score(img):
    """the score map of a level: 0 outside the candidate region and where the score is negative"""
    H, W = img.shape
    s = np.zeros((H, W), dtype=np.int64)
    if H < 2 * BORDER + 1 or W < 2 * BORDER + 1:
        return s
    B = BORDER
    p = img[B:H - B, B:W - B]
    d = np.stack([img[B + dy:H - B + dy, B + dx:W - B + dx] - p for dx, dy in RING])
    best = np.full(p.shape, -(1 << 20), dtype=np.int64)
    for k in range(16):
        arc = d[[(k + j) % 16 for j in range(9)]]
        best = np.maximum(best, np.maximum(arc.min(axis=0), (-arc).min(axis=0)))
    s[B:H - B, B:W - B] = np.maximum(best, 0)
    return s


def fast_score_literal(patch):
    """the largest threshold t at which the segment test passes at the centre of a 7 x 7 patch: 9 contiguous ring pixels all
    > p + t or all < p - t; -1 when it fails for t = 0 too.  Brute force over t (tests only)."""
    p = int(patch[3, 3])
    ring = [int(patch[3 + dy, 3 + dx]) for dx, dy in RING]
    best = -1
    for t in range(0, 256):
        ok = False
        for k in range(16):
            arc = [ring[(k + j) % 16] for j in range(9)]
            ok = ok or all(v > p + t for v in arc) or all(v < p - t for v in arc)
        if not ok:
            break
        best = t
    return best


def nms3(s, threshold):
    """pixel indices (ascending) of the corners that are the maximum of their 3 x 3 window under the raster tie rule"""
    H, W = s.shape
    keep = s > threshold
    p = np.pad(s, 1)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx == 0 and dy == 0:
                continue
            q = p[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
            keep &= (s > q) if (dy, dx) < (0, 0) else (s >= q)
    return np.flatnonzero(keep.reshape(-1))


def harris(img, xs, ys):
    Ix = (img[:, 2:] - img[:, :-2])
    Ix = Ix[:-2] + 2 * Ix[1:-1] + Ix[2:]           # at (y + 1, x + 1) of img
    Iy = (img[2:, :] - img[:-2, :])
    Iy = Iy[:, :-2] + 2 * Iy[:, 1:-1] + Iy[:, 2:]
    a = np.zeros(len(xs), dtype=np.int64)
    b, c = a.copy(), a.copy()
    for dy in range(-3, 4):
        for dx in range(-3, 4):
            gx, gy = Ix[ys + dy - 1, xs + dx - 1], Iy[ys + dy - 1, xs + dx - 1]
            a += gx * gx
            b += gy * gy
            c += gx * gy
    return 25 * (a * b - c * c) - (a + b) ** 2


def quotas(M, L):
    w = [5 ** l * 6 ** (L - 1 - l) for l in range(L)]
    q = [M * wl // sum(w) for wl in w]
    q[0] = M - sum(q[1:])
    return q


def level0_xy(x, y, W, H, Wl, Hl):
    return ((x.astype(np.float64) + 0.5) * float(W)) / float(Wl) - 0.5, ((y.astype(np.float64) + 0.5) * float(H)) / float(Hl) - 0.5


_DISC = [(u, v) for v in range(-15, 16) for u in range(-15, 16) if u * u + v * v <= 225]


def directions(img, xs, ys):
    m10 = np.zeros(len(xs), dtype=np.int64)
    m01 = m10.copy()
    for u, v in _DISC:
        I = img[ys + v, xs + u]
        m10 += u * I
        m01 += v * I
    val = np.stack([m10 * COS[k] + m01 * SIN[k] for k in range(32)])
    return np.argmax(val, axis=0).astype(np.int64), m10, m01     # argmax: the first maximum


def describe(blur, xs, ys, ks):
    tab = patterns()[ks]                                         # [n, 256, 4]
    va = blur[ys[:, None] + tab[:, :, 1], xs[:, None] + tab[:, :, 0]]
    vb = blur[ys[:, None] + tab[:, :, 3], xs[:, None] + tab[:, :, 2]]
    bits = (va < vb).astype(np.uint64).reshape(len(xs), 8, 32)
    words = (bits << np.arange(32, dtype=np.uint64)[None, None, :]).sum(axis=2).astype(np.uint32)
    return words.view(np.int32)


def orb_features(frame, max_features=500, levels=8, threshold=20, roi=None):
    M, L = int(max_features), int(levels)
    g, b = pyramid(frame, L)
    H, W = g[0].shape
    q = quotas(M, L)
    out = dict(xy_level=np.full((M, 2), -1, np.int32), xy=np.full((M, 2), -1.0), level=np.full(M, -1, np.int32),
               direction=np.full(M, -1, np.int32), score=np.zeros(M, np.int32), harris=np.zeros(M, np.int64),
               desc=np.zeros((M, 8), np.int32), level_count=np.zeros(L, np.int32))
    row = 0
    for l in range(L):
        Hl, Wl = g[l].shape
        s = fast_score(g[l])
        idx = nms3(s, threshold)
        ys, xs = idx // Wl, idx % Wl
        X, Y = level0_xy(xs, ys, W, H, Wl, Hl)
        if roi is not None:
            x1, y1, x2, y2 = (float(v) for v in roi)
            with np.errstate(invalid="ignore"):
                inside = (X >= x1) & (X < x2) & (Y >= y1) & (Y < y2)
            idx, xs, ys, X, Y = idx[inside], xs[inside], ys[inside], X[inside], Y[inside]
        out["level_count"][l] = len(idx)
        if len(idx) == 0:
            continue
        h = harris(g[l], xs, ys)
        order = np.lexsort((idx, -h))[:q[l]]
        sel = np.sort(order)                                     # idx ascends with its position
        xs, ys, X, Y, h = xs[sel], ys[sel], X[sel], Y[sel], h[sel]
        n = len(sel)
        ks, _, _ = directions(g[l], xs, ys)
        r = slice(row, row + n)
        out["xy_level"][r] = np.stack([xs, ys], axis=1)
        out["xy"][r] = np.stack([X, Y], axis=1)
        out["level"][r] = l
        out["direction"][r] = ks
        out["score"][r] = s[ys, xs]
        out["harris"][r] = h
        out["desc"][r] = describe(b[l], xs, ys, ks)
        row += n
    out["count"] = np.int32(row)
    return out


# ---- the matcher -----------------------------------------------------------------------------------------------------
_POP8 = np.array([bin(i).count("1") for i in range(256)], dtype=np.int64)


def hamming_matrix(d1, d2):
    a = np.ascontiguousarray(d1, dtype=np.int32).view(np.uint8).reshape(len(d1), 1, 32)
    b = np.ascontiguousarray(d2, dtype=np.int32).view(np.uint8).reshape(1, len(d2), 32)
    D = np.zeros((len(d1), len(d2)), dtype=np.int64)
    for i in range(0, len(d1), 64):                              # 64 rows at a time: the bytes' table is [64, n2, 32]
        D[i:i + 64] = _POP8[a[i:i + 64] ^ b].sum(axis=2)
    return D


def counting_sort_order(dist):
    """the order of a stable counting sort over the distances 0 .. 256: positions by (distance, index)"""
    hist = np.bincount(dist, minlength=257)
    start = np.concatenate([[0], np.cumsum(hist)[:-1]])
    order = np.zeros(len(dist), dtype=np.int64)
    for i, d in enumerate(dist):
        order[start[d]] = i
        start[d] += 1
    return order


def match_hamming(d1, d2, cross_check=True, ratio=None, max_distance=None, max_matches=1000):
    n1, n2, mm = len(d1), len(d2), int(max_matches)
    pairs, dist = np.full((mm, 2), -1, np.int32), np.full(mm, -1, np.int32)
    if n1 == 0 or n2 == 0:
        return pairs, dist, np.int32(0)
    D = hamming_matrix(d1, d2)
    j12 = np.argmin(D, axis=1)                                   # the first minimum: the smaller index on a tie
    i21 = np.argmin(D, axis=0)
    best = D[np.arange(n1), j12]
    keep = np.ones(n1, dtype=bool)
    if cross_check:
        keep &= i21[j12] == np.arange(n1)
    if ratio is not None:
        if n2 < 2:
            keep[:] = False
        else:
            D2 = D.copy()
            D2[np.arange(n1), j12] = 1 << 20
            second = D2.min(axis=1)
            keep &= best.astype(np.float64) < float(ratio) * second.astype(np.float64)
    if max_distance is not None:
        keep &= best <= int(max_distance)
    qi = np.flatnonzero(keep)
    qi = qi[counting_sort_order(best[qi])][:mm]
    pairs[:len(qi), 0], pairs[:len(qi), 1], dist[:len(qi)] = qi, j12[qi], best[qi]
    return pairs, dist, np.int32(len(qi))
