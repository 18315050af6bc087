"""NumPy restatement of the chessboard corner detector (DESIGN §2 "Chessboard corners"; the block in include/skimi.h):
rules 1-4 in int64 (exact: the kernels' int32 never overflows), rule 5 in float64 with every per-element expression
evaluated in the order csrc/chessboard.hip evaluates it (only the order of the five window sums differs), rules 6-8 through
the package's host code, which is NumPy already (calibration.order_chessboard is tested on its own on synthetic grids).

A frame is uint8 [H, W] or [H, W, ch], ch 1, 3 or 4 with colour channels in B, G, R order; points are (x, y).
"""
import numpy as np

RING = [(5, 0), (5, 2), (4, 4), (2, 5), (0, 5), (-2, 5), (-4, 4), (-5, 2),
        (-5, 0), (-5, -2), (-4, -4), (-2, -5), (0, -5), (2, -5), (4, -4), (5, -2)]
BORDER = 6


def ring_offsets():
    """rule 3's formula, which RING spells out"""
    k = np.arange(16)
    return [(int(np.rint(5 * np.cos(a))), int(np.rint(5 * np.sin(a)))) for a in k * np.pi / 8]


def gray(frame):
    """rule 1 -> int64 [H, W]"""
    f = np.asarray(frame)
    if f.ndim == 2:
        f = f[..., None]
    f = f.astype(np.int64)
    if f.shape[2] == 1:
        return f[..., 0]
    return (3735 * f[..., 0] + 19235 * f[..., 1] + 9798 * f[..., 2] + 16384) >> 15


def blur(g):
    """rule 2 -> int64 [H, W]; the outermost ring of pixels, which no response reads, is 0"""
    b = np.zeros_like(g)
    if g.shape[0] < 3 or g.shape[1] < 3:
        return b
    h = g[:, :-2] + 2 * g[:, 1:-1] + g[:, 2:]
    b[1:-1, 1:-1] = h[:-2] + 2 * h[1:-1] + h[2:]
    return b


def response(frame):
    """rule 3 -> int64 [H, W]"""
    b = blur(gray(frame))
    H, W = b.shape
    R = np.zeros((H, W), np.int64)
    if H <= 2 * BORDER or W <= 2 * BORDER:
        return R
    ys, xs = slice(BORDER, H - BORDER), slice(BORDER, W - BORDER)

    def at(dx, dy):
        return b[BORDER + dy:H - BORDER + dy, BORDER + dx:W - BORDER + dx]

    I = [at(dx, dy) for dx, dy in RING]
    sr = sum(np.abs(I[n] + I[n + 8] - I[n + 4] - I[n + 12]) for n in range(4))
    dr = sum(np.abs(I[n] - I[n + 8]) for n in range(8))
    c5 = at(0, 0) + at(-1, 0) + at(1, 0) + at(0, -1) + at(0, 1)
    R[ys, xs] = 5 * (sr - dr) - np.abs(5 * sum(I) - 16 * c5)
    return R


def candidates(frame, threshold=38, nms_radius=4, max_candidates=1024):
    """rule 4 -> dict(xy int32 [M, 2], response int32 [M], count, rmax)"""
    R = response(frame)
    H, W = R.shape
    rmax = int(R.max())
    r = int(nms_radius)
    keep = (R > 0) & (256 * R > int(threshold) * rmax)
    low = np.iinfo(np.int64).min
    pad = np.full((H + 2 * r, W + 2 * r), low, np.int64)
    pad[r:r + H, r:r + W] = R
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            if dx == 0 and dy == 0:
                continue
            q = pad[r + dy:r + dy + H, r + dx:r + dx + W]
            keep &= (R > q) if (dy, dx) < (0, 0) else (R >= q)      # an earlier pixel in raster order: strictly greater
    ys, xs = np.nonzero(keep)                                       # ascending pixel order
    M = int(max_candidates)
    xy, resp = np.full((M, 2), -1, np.int32), np.zeros(M, np.int32)
    k = min(len(ys), M)
    xy[:k, 0], xy[:k, 1], resp[:k] = xs[:k], ys[:k], R[ys[:k], xs[:k]]
    return {"xy": xy, "response": resp, "count": np.int32(len(ys)), "rmax": np.int32(rmax)}


def corner_subpix(frame, points, count=None, win=(5, 5), iters=30):
    """rule 5 -> (points float64 [M, 2], ok bool [M])"""
    g = gray(frame).astype(np.float64)
    H, W = g.shape
    wx, wy = (int(w) for w in win)
    pts = np.asarray(points, np.float64).reshape(-1, 2)
    n = len(pts) if count is None else min(int(count), len(pts))
    out, ok = pts.copy(), np.zeros(len(pts), bool)
    jj, ii = np.arange(2 * wx + 1), np.arange(2 * wy + 1)
    ux, uy = (jj - wx) / float(wx), (ii - wy) / float(wy)
    m = np.exp(-(ux * ux))[None, :] * np.exp(-(uy * uy))[:, None]
    qx, qy = (jj - wx).astype(np.float64)[None, :], (ii - wy).astype(np.float64)[:, None]
    for k in range(n):
        x0, y0 = pts[k]
        if not (x0 >= 0.0 and x0 < W and y0 >= 0.0 and y0 < H):
            continue
        x, y = x0, y0
        for _ in range(int(iters)):
            fx, fy = np.floor(x), np.floor(y)
            a, b = x - fx, y - fy
            cx = np.clip(int(fx) - wx - 1 + np.arange(2 * wx + 4), 0, W - 1)
            cy = np.clip(int(fy) - wy - 1 + np.arange(2 * wy + 4), 0, H - 1)
            foot = g[np.ix_(cy, cx)]
            p = (1.0 - b) * ((1.0 - a) * foot[:-1, :-1] + a * foot[:-1, 1:]) + b * ((1.0 - a) * foot[1:, :-1] + a * foot[1:, 1:])
            gx = p[1:-1, 2:] - p[1:-1, :-2]
            gy = p[2:, 1:-1] - p[:-2, 1:-1]
            gxx, gxy, gyy = (gx * gx) * m, (gx * gy) * m, (gy * gy) * m
            A, B, C = gxx.sum(), gxy.sum(), gyy.sum()
            bb1, bb2 = (gxx * qx + gxy * qy).sum(), (gxy * qx + gyy * qy).sum()
            det = A * C - B * B
            if det == 0.0 or not np.isfinite(det):
                break
            x, y = x + (C * bb1 - B * bb2) / det, y + (A * bb2 - B * bb1) / det
            if not (x >= 0.0 and x < W and y >= 0.0 and y < H):
                break
        if abs(x - x0) <= wx and abs(y - y0) <= wy:
            out[k], ok[k] = (x, y), True
    return out, ok


def find_chessboard_corners(frame, board_size, win=(5, 5), threshold=38, nms_radius=4, max_candidates=1024, iters=30):
    """rules 1-8 on one frame -> (corners [cols * rows, 2] or None, the candidates' dict, the refined points, ok)"""
    from skiing_analysis_pytorch_amd import calibration
    c = candidates(frame, threshold, nms_radius, max_candidates)
    k = min(int(c["count"]), int(max_candidates))
    pts, ok = corner_subpix(frame, c["xy"][:k], win=win, iters=iters)
    board = calibration.order_chessboard(pts[ok], board_size, strength=c["response"][:k][ok])
    return board, c, pts, ok
