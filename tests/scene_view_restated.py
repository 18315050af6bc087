"""NumPy restatement of the scene-view renderer (include/skimi.h, "3D scene views") and of its builders, and a brute-force
painter written differently (per pixel: every fragment, sorted by (w, rank)) that checks the restatement itself."""
import math

import numpy as np

W_ONE = 1 << 30
SAT = 1 << 20
NONE, DISC, CAPSULE = 0, 1, 2


# ---- rule 1: the projection of points ---------------------------------------------------------------------------------------
def project(view, xyz):
    """view [20] f64, xyz [n, 3] -> ok, u, v, w (f64 arrays; w clamped), in the header's operation order"""
    V = np.asarray(view, dtype=np.float64)
    p = np.asarray(xyz).astype(np.float64).reshape(-1, 3)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        X = ((V[0] * x + V[1] * y) + V[2] * z) + V[3]
        Y = ((V[4] * x + V[5] * y) + V[6] * z) + V[7]
        Z = ((V[8] * x + V[9] * y) + V[10] * z) + V[11]
        near, far = V[16], V[17]
        ok = np.isfinite(X) & np.isfinite(Y) & np.isfinite(Z) & (Z >= near) & (Z <= far)
        if V[18] != 0:
            u, v = V[12] * X + V[14], V[13] * Y + V[15]
            q = np.floor((float(W_ONE) * (far - Z)) / (far - near))
        else:
            ok &= Z > 0
            u, v = (V[12] * X) / Z + V[14], (V[13] * Y) / Z + V[15]
            q = np.floor((float(W_ONE) * near) / Z)
        q = np.minimum(np.where(q >= 1.0, q, 1.0), float(W_ONE))
    return ok, u, v, q


def decode_depth(view, w):
    """rule 4: w (int array, 0 = empty) -> float32 Z, +inf where empty"""
    V = np.asarray(view, dtype=np.float64)
    near, far = V[16], V[17]
    wf = np.where(w > 0, w, 1).astype(np.float64)
    with np.errstate(all="ignore"):
        Z = far - (wf * (far - near)) / float(W_ONE) if V[18] != 0 else (float(W_ONE) * near) / wf
    return np.where(w > 0, Z, np.inf).astype(np.float32)


def splat(view, xyz, size, H, W):
    """rule 2: the key buffer u64 [H, W] of one frame"""
    keys = np.zeros((H, W), dtype=np.uint64)
    n = len(xyz)
    if n == 0:
        return keys
    ok, u, v, q = project(view, xyz)
    with np.errstate(all="ignore"):
        fu, fv = np.floor(u) - (size - 1) // 2, np.floor(v) - (size - 1) // 2      # the square's first pixel
        ok = ok & (fu > -size) & (fu < W) & (fv > -size) & (fv < H)
    i = np.nonzero(ok)[0]
    key = (q[i].astype(np.uint64) << np.uint64(32)) | i.astype(np.uint64)
    px, py = fu[i].astype(np.int64), fv[i].astype(np.int64)
    for dy in range(size):
        for dx in range(size):
            xx, yy = px + dx, py + dy
            m = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
            np.maximum.at(keys, (yy[m], xx[m]), key[m])
    return keys


# ---- rule 3: primitives -----------------------------------------------------------------------------------------------------
def read_prim(rec):
    """a record as the rules read it -> (kind, x0, y0, x1, y1, r, colour, w0, w1) Python ints"""
    kind, x0, y0, x1, y1, r, colour, w0, w1 = (int(v) for v in rec[:9])
    sat = lambda v: min(max(v, -SAT), SAT)   # noqa: E731
    cw = lambda v: min(max(v, 1), W_ONE)     # noqa: E731
    x0, y0, x1, y1, r, w0, w1 = sat(x0), sat(y0), sat(x1), sat(y1), sat(r), cw(w0), cw(w1)
    if kind not in (DISC, CAPSULE):
        kind = NONE
    if kind == DISC:
        x1, y1, w1 = x0, y0, w0
    return kind, x0, y0, x1, y1, r, colour & 0xFFFFFF, w0, w1


def _isqrt(n):
    r = np.floor(np.sqrt(n.astype(np.float64))).astype(np.int64)
    r = r - (r * r > n)
    return r + ((r + 1) * (r + 1) <= n)


def fragment_map(rec, H, W):
    """the w of the primitive's fragment at every pixel, int64 [H, W], 0 where the centre is not covered"""
    kind, x0, y0, x1, y1, r, _, w0, w1 = read_prim(rec)
    if kind == NONE or r < 0:
        return np.zeros((H, W), dtype=np.int64)
    U, V = np.meshgrid(np.arange(W, dtype=np.int64), np.arange(H, dtype=np.int64))
    px, py = 16 * U - x0, 16 * V - y0
    ex, ey = x1 - x0, y1 - y0
    L2 = ex * ex + ey * ey
    da = _isqrt(px * px + py * py)
    if L2 == 0:
        return np.where(da <= r, w0, 0)
    t = px * ex + py * ey
    root = math.isqrt(L2)
    db = _isqrt((px - ex) ** 2 + (py - ey) ** 2)
    dl = np.abs(px * ey - py * ex) // root
    inside = (t > 0) & (t < L2)
    ti = np.where(inside, t, 0)
    m = abs(w1 - w0)
    rem, Q = np.zeros_like(t), np.zeros_like(t)
    for k in (3, 2, 1, 0):              # long division in base 256: every intermediate below 2^52
        acc = rem * 256 + ((m >> (8 * k)) & 255) * ti
        q = acc // L2
        rem, Q = acc - q * L2, Q * 256 + q
    wl = w0 + Q if w1 >= w0 else w0 - Q
    d = np.where(t <= 0, da, np.where(t >= L2, db, dl))
    w = np.where(t <= 0, w0, np.where(t >= L2, w1, wl))
    return np.where(d <= r, w, 0)


# ---- rule 4: the frame ------------------------------------------------------------------------------------------------------
def _defaults(F, xyz, count, cof):
    P = 0 if xyz is None else xyz.shape[0]
    N = 0 if xyz is None else xyz.shape[1]
    n = [N] * P if count is None else [min(max(int(c), 0), N) for c in count]
    if cof is None:
        cof = [0] * F if P == 1 else list(range(F))
    return P, n, [int(c) for c in cof]


def background_frames(background, F, H, W):
    if isinstance(background, np.ndarray) and background.ndim == 4:
        return background.copy()
    c = [int(background)] * 3 if np.isscalar(background) else [int(v) for v in background]
    return np.broadcast_to(np.array(c, dtype=np.uint8), (F, H, W, 3)).copy()


def render(views, xyz, rgb, count, cof, point_size, prims, H, W, background=0):
    """-> frames u8 [F, H, W, 3], depth f32 [F, H, W], index i32 [F, H, W]"""
    F = len(views)
    P, n, cof = _defaults(F, xyz, count, cof)
    frames = background_frames(background, F, H, W)
    depth, index = np.zeros((F, H, W), dtype=np.float32), np.zeros((F, H, W), dtype=np.int32)
    for f in range(F):
        p = cof[f]
        has = 0 <= p < P
        keys = splat(views[f], xyz[p, :n[p]], point_size, H, W) if has else np.zeros((H, W), dtype=np.uint64)
        bw = (keys >> np.uint64(32)).astype(np.int64)
        idx = (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
        index[f] = np.where(keys > 0, idx, -1)
        if has and n[p]:
            frames[f][keys > 0] = rgb[p][idx[keys > 0]]
        recs = np.zeros((0, 12), dtype=np.int32) if prims is None else (prims if prims.ndim == 2 else prims[f])
        for rec in recs:
            wm = fragment_map(rec, H, W)
            take = (wm > 0) & (wm >= bw)
            bw = np.where(take, wm, bw)
            c = read_prim(rec)[6]
            frames[f][take] = [c & 255, (c >> 8) & 255, (c >> 16) & 255]
        depth[f] = decode_depth(views[f], bw)
    return frames, depth, index


# ---- the brute-force painter ------------------------------------------------------------------------------------------------
def _prim_fragment_int(prim, u, v):
    """one primitive at one pixel in Python integers: w or 0"""
    kind, x0, y0, x1, y1, r, _, w0, w1 = prim
    px, py, ex, ey = 16 * u - x0, 16 * v - y0, x1 - x0, y1 - y0
    L2 = ex * ex + ey * ey
    t = px * ex + py * ey
    if L2 == 0 or t <= 0:
        return w0 if math.isqrt(px * px + py * py) <= r else 0
    if t >= L2:
        return w1 if math.isqrt((px - ex) ** 2 + (py - ey) ** 2) <= r else 0
    if abs(px * ey - py * ex) // math.isqrt(L2) > r:
        return 0
    step = (abs(w1 - w0) * t) // L2          # big integers: no limbs needed
    return w0 + step if w1 >= w0 else w0 - step


def paint_brute(views, xyz, rgb, count, cof, point_size, prims, H, W, background=0):
    """Every fragment of every pixel collected as (w, rank, colour, point index), rank = the point's index, or N + the
    primitive's list position; the winner is the largest (w, rank).  -> frames, depth, index as render."""
    F = len(views)
    P, n, cof = _defaults(F, xyz, count, cof)
    N = 0 if xyz is None else xyz.shape[1]
    frames = background_frames(background, F, H, W)
    depth, index = np.full((F, H, W), np.inf, dtype=np.float32), np.full((F, H, W), -1, dtype=np.int32)
    for f in range(F):
        frags = {}
        p = cof[f]
        if 0 <= p < P and n[p]:
            ok, u, v, q = project(views[f], xyz[p, :n[p]])
            for i in np.nonzero(ok)[0]:
                if not (math.isfinite(u[i]) and math.isfinite(v[i])) or abs(u[i]) > 1e6 or abs(v[i]) > 1e6:
                    continue
                bx, by = math.floor(u[i]) - (point_size - 1) // 2, math.floor(v[i]) - (point_size - 1) // 2
                for yy in range(max(by, 0), min(by + point_size, H)):
                    for xx in range(max(bx, 0), min(bx + point_size, W)):
                        frags.setdefault((yy, xx), []).append((int(q[i]), int(i), tuple(int(c) for c in rgb[p][i]), int(i)))
        recs = [] if prims is None else (prims if prims.ndim == 2 else prims[f])
        for k, rec in enumerate(recs):
            prim = read_prim(rec)
            kind, x0, y0, x1, y1, r, c, _, _ = prim
            if kind == NONE or r < 0:
                continue
            lo_x, hi_x = max((min(x0, x1) - r) // 16 - 1, 0), min((max(x0, x1) + r) // 16 + 2, W)
            lo_y, hi_y = max((min(y0, y1) - r) // 16 - 1, 0), min((max(y0, y1) + r) // 16 + 2, H)
            for yy in range(lo_y, hi_y):
                for xx in range(lo_x, hi_x):
                    w = _prim_fragment_int(prim, xx, yy)
                    if w:
                        frags.setdefault((yy, xx), []).append((w, N + k, (c & 255, (c >> 8) & 255, (c >> 16) & 255), -1))
        for (yy, xx), lst in frags.items():
            lst.sort(key=lambda e: (e[0], e[1]))
            frames[f, yy, xx] = lst[-1][2]
            depth[f, yy, xx] = decode_depth(views[f], np.array([lst[-1][0]]))[0]
            pts = [e for e in lst if e[3] >= 0]
            if pts:
                index[f, yy, xx] = pts[-1][3]
    return frames, depth, index


# ---- the builders, restated -------------------------------------------------------------------------------------------------
def look_at(eye, target, up, fx, fy, cx, cy, near, far, ortho=False):
    eye, target, up = (np.asarray(a, dtype=np.float64) for a in (eye, target, up))
    fwd = (target - eye) / np.linalg.norm(target - eye)
    right = np.cross(fwd, up)
    right = right / np.linalg.norm(right)
    down = np.cross(fwd, right)
    R = np.stack([right, down, fwd])
    return np.concatenate([np.concatenate([R, (-R @ eye)[:, None]], axis=1).reshape(-1), [fx, fy, cx, cy, near, far, float(ortho), 0.0]])


def orbit_eye(center, radius, elev_deg, azim_deg):
    el, az = math.radians(elev_deg), math.radians(azim_deg)
    return np.asarray(center, dtype=np.float64) + radius * np.array([math.cos(el) * math.cos(az), math.cos(el) * math.sin(az), math.sin(el)])


def to_camera(view, p):
    V = np.asarray(view, dtype=np.float64)
    M = V[:12].reshape(3, 4)
    return M[:, :3] @ np.asarray(p, dtype=np.float64) + M[:, 3]        # a matrix product: another operation order


def project_camera(view, c):
    """camera-frame point -> (u, v, w) or None"""
    V = np.asarray(view, dtype=np.float64)
    near, far = V[16], V[17]
    X, Y, Z = c
    if not np.isfinite(c).all() or Z < near or Z > far:
        return None
    if V[18] != 0:
        u, v, q = V[12] * X + V[14], V[13] * Y + V[15], math.floor(W_ONE * ((far - Z) / (far - near)))
    else:
        if Z <= 0:
            return None
        u, v, q = V[12] * (X / Z) + V[14], V[13] * (Y / Z) + V[15], math.floor(W_ONE * (near / Z))
    return u, v, min(max(q, 1), W_ONE)


def grid(u):
    return int(np.round((u - 0.5) * 16.0))


def disc_prim(view, p, colour, radius_px):
    pr = project_camera(view, to_camera(view, p)) if np.isfinite(p).all() else None
    if pr is None:
        return np.zeros(12, dtype=np.int64)
    u, v, w = pr
    return np.array([DISC, grid(u), grid(v), grid(u), grid(v), int(np.round(radius_px * 16)), colour, w, w, 0, 0, 0], dtype=np.int64)


def clip_segment(a, b, near):
    """camera-frame ends -> (a, b) clipped to Z >= near, or None when wholly behind"""
    a, b = np.array(a, dtype=np.float64), np.array(b, dtype=np.float64)
    if a[2] < near and b[2] < near:
        return None
    if a[2] < near or b[2] < near:
        s = (near - a[2]) / (b[2] - a[2])
        c = a + s * (b - a)
        c[2] = near
        if a[2] < near:
            a = c
        else:
            b = c
    return a, b


def segment_prim(view, p0, p1, colour, thickness_px):
    none = np.zeros(12, dtype=np.int64)
    if not (np.isfinite(p0).all() and np.isfinite(p1).all()):
        return none
    ends = clip_segment(to_camera(view, p0), to_camera(view, p1), view[16])
    if ends is None:
        return none
    pa, pb = project_camera(view, ends[0]), project_camera(view, ends[1])
    if pa is None or pb is None:
        return none
    return np.array([CAPSULE, grid(pa[0]), grid(pa[1]), grid(pb[0]), grid(pb[1]), int(np.round(thickness_px * 8)), colour, pa[2], pb[2],
                     0, 0, 0], dtype=np.int64)
