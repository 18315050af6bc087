"""NumPy restatement of the SIFT-style feature rules (include/skimi.h "SIFT-style image features", DESIGN §2 "Image features
(SIFT-style)"), written from the rules and not from csrc/sift.hip: the scale space in float32 in the kernel's operation order,
the refinement in float64 with the same elementary operations (Python floats), orientation and descriptor in float64 on
whole windows.

    sift_features(frame, max_features, octaves, roi) -> dict of the outputs of geometry.sift_features for one frame, and
                                                        desc_value (512 v ahead of the rounding), margin (the relative gap
                                                        between the two highest smoothed orientation bins)
    match_l2(d1, d2, ...)                            -> (pairs, dist2, second2, count) for one pair of descriptor sets
"""
import math

import numpy as np

import features_restated as fr

S, SIGMA0, BORDER, MIN_SIDE, MAX_OCTAVES, MAX_CANDIDATES = 3, 1.6, 5, 16, 8, 32768
PRETHRESH = np.float32(1.7)
CONTRAST = 3.4
CBRT4, LN2 = 1.5874010519681994, 0.6931471805599453
TWO_PI = 6.283185307179586


# ---- the scale space ---------------------------------------------------------------------------------------------
def sigmas():
    k = 2.0 ** (1.0 / S)
    return [math.sqrt(SIGMA0 * SIGMA0 - 0.25)] + [SIGMA0 * k ** (i - 1) * math.sqrt(k * k - 1.0) for i in range(1, S + 3)]


def taps64(sigma):
    """the float64 taps of a blur, radius ceil(4 sigma), normalised"""
    r = int(math.ceil(4.0 * sigma))
    x = np.arange(-r, r + 1, dtype=np.float64)
    g = np.exp(-(x * x) / (2.0 * sigma * sigma))
    return g / g.sum()


def taps():
    return [taps64(s).astype(np.float32) for s in sigmas()]


def blur(img, t):
    """horizontal then vertical, float32 products added in tap order from the first product, borders replicated"""
    r = (len(t) - 1) // 2
    H, W = img.shape
    p = np.pad(img, ((0, 0), (r, r)), mode="edge")
    acc = t[0] * p[:, 0:W]
    for k in range(1, 2 * r + 1):
        acc = acc + t[k] * p[:, k:k + W]
    p = np.pad(acc, ((r, r), (0, 0)), mode="edge")
    out = t[0] * p[0:H, :]
    for k in range(1, 2 * r + 1):
        out = out + t[k] * p[k:k + H, :]
    assert out.dtype == np.float32
    return out


def default_octaves(H, W):
    n = 0
    while n < MAX_OCTAVES and min(H, W) >= MIN_SIDE:
        n, H, W = n + 1, (H + 1) // 2, (W + 1) // 2
    return n


def scale_space(frame, octaves):
    """a list of [6, H_o, W_o] float32 arrays, the octaves that are not empty"""
    t = taps()
    base = fr.gray(frame).astype(np.float32)
    out = []
    for o in range(octaves):
        if min(base.shape) < MIN_SIDE:
            break
        layers = [blur(base, t[0])] if o == 0 else [base]
        for i in range(1, S + 3):
            layers.append(blur(layers[-1], t[i]))
        out.append(np.stack(layers))
        base = layers[S][::2, ::2]
    return out


def candidates(dog, l):
    """pixel indices (ascending) of the strict 26-neighbour extrema of DoG layer l"""
    _, H, W = dog.shape
    B = BORDER
    c = dog[l, B:H - B, B:W - B]
    mx = np.abs(c) > PRETHRESH
    mn = mx.copy()
    for dl in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if dl == 0 and dy == 0 and dx == 0:
                    continue
                q = dog[l + dl, B + dy:H - B + dy, B + dx:W - B + dx]
                mx &= c > q
                mn &= c < q
    ys, xs = np.nonzero(mx | mn)
    return (ys + B) * W + (xs + B)


# ---- refinement: Python floats are IEEE doubles, every operation is written out ----------------------------------
def refine(dog, o, l, x, y, roi=None):
    """-> None, or (X, Y, sigma, response, x, y, l)"""
    _, H, W = dog.shape
    D = lambda l_, y_, x_: float(dog[l_, y_, x_])   # noqa: E731
    for _ in range(5):
        v = D(l, y, x)
        g0 = (D(l, y, x + 1) - D(l, y, x - 1)) * 0.5
        g1 = (D(l, y + 1, x) - D(l, y - 1, x)) * 0.5
        g2 = (D(l + 1, y, x) - D(l - 1, y, x)) * 0.5
        v2 = 2.0 * v
        dxx = D(l, y, x + 1) + D(l, y, x - 1) - v2
        dyy = D(l, y + 1, x) + D(l, y - 1, x) - v2
        dss = D(l + 1, y, x) + D(l - 1, y, x) - v2
        dxy = (D(l, y + 1, x + 1) - D(l, y + 1, x - 1) - D(l, y - 1, x + 1) + D(l, y - 1, x - 1)) * 0.25
        dxs = (D(l + 1, y, x + 1) - D(l + 1, y, x - 1) - D(l - 1, y, x + 1) + D(l - 1, y, x - 1)) * 0.25
        dys = (D(l + 1, y + 1, x) - D(l + 1, y - 1, x) - D(l - 1, y + 1, x) + D(l - 1, y - 1, x)) * 0.25
        b0, b1, b2 = -g0, -g1, -g2
        with np.errstate(all="ignore"):
            dv = lambda a, b: float(np.float64(a) / np.float64(b))   # noqa: E731  (x / 0 is inf or NaN, not an exception)
            m10, m20 = dv(dxy, dxx), dv(dxs, dxx)
            a11, a12, c1 = dyy - m10 * dxy, dys - m10 * dxs, b1 - m10 * b0
            a21, a22, c2 = dys - m20 * dxy, dss - m20 * dxs, b2 - m20 * b0
            m21 = dv(a21, a11)
            e22, e2 = a22 - m21 * a12, c2 - m21 * c1
            X2 = dv(e2, e22)
            X1 = dv(c1 - a12 * X2, a11)
            X0 = dv(b0 - dxy * X1 - dxs * X2, dxx)
        mx = 1 if X0 > 0.5 else (-1 if X0 < -0.5 else 0)
        my = 1 if X1 > 0.5 else (-1 if X1 < -0.5 else 0)
        ml = 1 if X2 > 0.5 else (-1 if X2 < -0.5 else 0)
        if mx == 0 and my == 0 and ml == 0:
            break
        x, y, l = x + mx, y + my, l + ml
        if l < 1 or l > S or x < BORDER or x >= W - BORDER or y < BORDER or y >= H - BORDER:
            return None
    else:
        return None
    resp = v + ((g0 * X0 + g1 * X1) + g2 * X2) * 0.5
    tr, det = dxx + dyy, dxx * dyy - dxy * dxy
    if not (abs(resp) >= CONTRAST) or not (det > 0.0) or not (tr * tr * 10.0 < 121.0 * det):
        return None
    scale = float(1 << o)
    X, Y = (float(x) + X0) * scale, (float(y) + X1) * scale
    z = ((float(l) + X2) / 3.0 - 2.0 / 3.0) * LN2
    p = 1.0
    for k in range(16, 0, -1):
        p = 1.0 + z * p / float(k)
    sigma = 1.6 * scale * CBRT4 * p
    if roi is not None:
        x1, y1, x2, y2 = (float(t) for t in roi)
        if not (X >= x1 and X < x2 and Y >= y1 and Y < y2):
            return None
    return X, Y, sigma, resp, x, y, l


# ---- orientation and descriptor in float64 -----------------------------------------------------------------------
def _window(L, x, y, R):
    """offsets (i along y, j along x) of the window of half side R whose pixels have all four neighbours; gx, gy there"""
    H, W = L.shape
    i, j = np.mgrid[-R:R + 1, -R:R + 1]
    px, py = x + j, y + i
    ok = (px >= 1) & (px <= W - 2) & (py >= 1) & (py <= H - 2)
    i, j, px, py = i[ok], j[ok], px[ok], py[ok]
    L64 = L.astype(np.float64)
    return i.astype(np.float64), j.astype(np.float64), L64[py, px + 1] - L64[py, px - 1], L64[py + 1, px] - L64[py - 1, px]


def smooth(h):
    return ((np.roll(h, 2) + np.roll(h, -2)) + 4.0 * (np.roll(h, 1) + np.roll(h, -1)) + 6.0 * h) / 16.0


def orientation(L, x, y, s):
    """-> (angle in [0, 2 pi), the relative gap between the two highest smoothed bins)"""
    rad = 4.5 * s
    i, j, gx, gy = _window(L, x, y, int(math.floor(rad)))
    ok = (i * i + j * j) <= rad * rad
    i, j, gx, gy = i[ok], j[ok], gx[ok], gy[ok]
    w = np.sqrt(gx * gx + gy * gy) * np.exp(-(i * i + j * j) / (2.0 * (1.5 * s) * (1.5 * s)))
    th = np.arctan2(gy, gx)
    th = np.where(th < 0.0, th + TWO_PI, th)
    fb = th * 36.0 / TWO_PI
    b0 = np.floor(fb)
    f = fb - b0
    k0 = b0.astype(np.int64) % 36
    h = np.zeros(36)
    np.add.at(h, k0, w * (1.0 - f))
    np.add.at(h, (k0 + 1) % 36, w * f)
    h = smooth(smooth(h))
    k = int(np.argmax(h))                          # the first maximum
    top = np.sort(h)
    margin = (top[-1] - top[-2]) / top[-1] if top[-1] > 0 else 0.0
    l, r = h[(k + 35) % 36], h[(k + 1) % 36]
    dn = l - 2.0 * h[k] + r
    p = k + (0.5 * (l - r) / dn if dn != 0.0 else 0.0)
    a = TWO_PI * p / 36.0
    if a < 0.0:
        a += TWO_PI
    if a >= TWO_PI:
        a -= TWO_PI
    return a, float(margin)


def descriptor(L, x, y, s, angle):
    """-> (512 v ahead of the rounding [128], bytes [128])"""
    hw = 3.0 * s
    R = int(math.floor(hw * 1.4142135623730951 * 2.5 + 0.5))
    i, j, gx, gy = _window(L, x, y, R)
    ca, sa = math.cos(angle), math.sin(angle)
    c, r = (ca * j + sa * i) / hw, (-sa * j + ca * i) / hw
    rb, cb = r + 1.5, c + 1.5
    ok = (rb > -1.0) & (rb < 4.0) & (cb > -1.0) & (cb < 4.0)
    c, r, rb, cb, gx, gy = c[ok], r[ok], rb[ok], cb[ok], gx[ok], gy[ok]
    ob = (np.arctan2(gy, gx) - angle) * 8.0 / TWO_PI
    ob = ob - np.floor(ob / 8.0) * 8.0
    val = np.sqrt(gx * gx + gy * gy) * np.exp(-(r * r + c * c) / 8.0)
    r0, c0, o0 = np.floor(rb), np.floor(cb), np.floor(ob)
    fr_, fc, fo = rb - r0, cb - c0, ob - o0
    r0, c0, o0 = r0.astype(np.int64), c0.astype(np.int64), o0.astype(np.int64)
    v = np.zeros(128)
    for dr in (0, 1):
        for dc in (0, 1):
            for do in (0, 1):
                row, col = r0 + dr, c0 + dc
                inside = (row >= 0) & (row <= 3) & (col >= 0) & (col <= 3)
                wgt = val * (fr_ if dr else 1.0 - fr_) * (fc if dc else 1.0 - fc) * (fo if do else 1.0 - fo)
                np.add.at(v, ((row * 4 + col) * 8 + ((o0 + do) & 7))[inside], wgt[inside])
    n = math.sqrt(float((v * v).sum()))
    if not n > 0.0:
        return np.zeros(128), np.zeros(128, np.uint8)
    v = np.minimum(v / n, 0.2)
    v = 512.0 * (v / math.sqrt(float((v * v).sum())))
    return v, np.minimum(255, np.rint(v)).astype(np.uint8)      # rint: round half to even


def sift_features(frame, max_features=3000, octaves=None, roi=None):
    M = int(max_features)
    H, W = np.asarray(frame).shape[:2]
    O = default_octaves(H, W) if octaves is None else int(octaves)
    gauss = scale_space(frame, O)
    out = dict(xy=np.full((M, 2), -1.0), xy_level=np.full((M, 2), -1, np.int32), octave=np.full(M, -1, np.int32),
               layer=np.full(M, -1, np.int32), sigma=np.zeros(M), response=np.zeros(M), angle=np.full(M, -1.0),
               desc=np.zeros((M, 128), np.uint8), octave_count=np.zeros(O, np.int32), desc_value=np.zeros((M, 128)),
               margin=np.full(M, np.inf))
    kept = []                                                   # in candidate order
    for o, g in enumerate(gauss):
        dog = g[1:] - g[:-1]
        Wo = g.shape[2]
        for l in range(1, S + 1):
            idx = candidates(dog, l)
            out["octave_count"][o] += len(idx)
            for p in idx[:min(g.shape[1] * Wo, MAX_CANDIDATES)]:
                ref = refine(dog, o, l, int(p % Wo), int(p // Wo), roi)
                if ref is not None:
                    kept.append((o,) + ref)
    if len(kept) > M:
        key = np.array([abs(k[4]) for k in kept])
        order = np.lexsort((np.arange(len(kept)), -key))[:M]   # the largest |response|, ties to the earlier candidate
        kept = [kept[i] for i in np.sort(order)]
    for row, (o, X, Y, sigma, resp, x, y, l) in enumerate(kept):
        s = sigma / float(1 << o)
        angle, margin = orientation(gauss[o][l], x, y, s)
        value, byte = descriptor(gauss[o][l], x, y, s, angle)
        out["xy"][row], out["xy_level"][row], out["octave"][row], out["layer"][row] = (X, Y), (x, y), o, l
        out["sigma"][row], out["response"][row], out["angle"][row], out["margin"][row] = sigma, resp, angle, margin
        out["desc"][row], out["desc_value"][row] = byte, value
    out["count"] = np.int32(len(kept))
    return out


# ---- the matcher -------------------------------------------------------------------------------------------------
def l2_matrix(d1, d2):
    """exact squared distances in int64"""
    a, b = np.asarray(d1).astype(np.int64), np.asarray(d2).astype(np.int64)
    return (a * a).sum(axis=1)[:, None] + (b * b).sum(axis=1)[None, :] - 2 * (a @ b.T)


def match_l2(d1, d2, ratio=0.75, cross_check=False, max_distance2=None, max_matches=1000):
    n1, n2, mm = len(d1), len(d2), int(max_matches)
    pairs, dist2, second2 = np.full((mm, 2), -1, np.int32), np.full(mm, -1, np.int32), np.full(mm, -1, np.int32)
    if n1 == 0 or n2 == 0:
        return pairs, dist2, second2, np.int32(0)
    D = l2_matrix(d1, d2)
    j12 = np.argmin(D, axis=1)                                   # the first minimum: the smaller index on a tie
    i21 = np.argmin(D, axis=0)
    s1 = D[np.arange(n1), j12]
    s2 = np.full(n1, -1, np.int64)
    if n2 >= 2:
        D2 = D.copy()
        D2[np.arange(n1), j12] = 1 << 40
        s2 = D2.min(axis=1)                                      # may equal s1
    keep = np.ones(n1, dtype=bool)
    if cross_check:
        keep &= i21[j12] == np.arange(n1)
    if ratio is not None:
        r = float(ratio)
        keep &= (s1.astype(np.float64) < (r * r) * s2.astype(np.float64)) if n2 >= 2 else False
    if max_distance2 is not None:
        keep &= s1 <= int(max_distance2)
    qi = np.flatnonzero(keep)
    qi = qi[np.argsort(s1[qi], kind="stable")][:mm]              # by (s1, query)
    n = len(qi)
    pairs[:n, 0], pairs[:n, 1], dist2[:n], second2[:n] = qi, j12[qi], s1[qi], s2[qi]
    return pairs, dist2, second2, np.int32(n)
