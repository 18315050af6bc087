"""Inputs of the chessboard detector's tests: boards rendered through the full rational lens of tests/golden/calibrate.npz
(camera matrix, 8 coefficients, 24 board poses) at a third of its scale, 640 x 360, with the truth from
lens_restated.project_points.

Every pixel is supersampled SS x SS; each sample goes through lens_restated.undistort_points (normalised) to its ray and on
to the board's plane.  The checker is 30 / 220 with a one-square white margin on a 128 background.  Only the window around
the board is traced (the rest is background), which keeps a frame at about a second of CPU; frames are cached per session.
"""
import functools

import numpy as np

import calibrate_cases as cc
import chessboard_restated as cs
import lens_restated as lr

SCALE = 3
SIZE = (1920 // SCALE, 1080 // SCALE)     # (width, height)
BOARD = (9, 6)
VIEWS = (0, 9, 13)                        # steps of roughly 19-33 px at this scale: every path in seconds
CALIB_VIEWS = (0, 5, 9, 13, 18, 21)       # six views for calibrate_from_frames
SS = 3
DARK, LIGHT, BACK = 30, 220, 128
WIN = (5, 5)   # at this scale the reference's (11, 11) window holds the neighbouring corners: profiles/chessboard.md

# Accuracy against the rendered truth cannot be derived: it was measured on the CPU with the restatement, worst and mean corner
# error per rendered case (profiles/chessboard.md, "Accuracy against the rendered truth").  The worst corner of the cases these
# tests use (views 0, 5, 9, 13, 18, 21 at WIN) is 0.295 px, in view 13; the bound is twice that, because the error depends on the
# board's step and on the lens curvature inside the window, which vary from view to view.
TRUTH_BOUND_PX = 0.59


def camera(shift=(0.0, 0.0)):
    """the fixture's K at 1 / SCALE (principal point moved by `shift` pixels) and its eight coefficients"""
    f = cc.fixture()
    K = f["camera_matrix"].astype(np.float64) / SCALE
    K[2, 2] = 1.0
    K[0, 2] += shift[0]
    K[1, 2] += shift[1]
    return K, f["dist_coeffs"][:8].astype(np.float64), f


def truth(view, shift=(0.0, 0.0)):
    """the 54 inner corners' pixels, row-major like prepare_object_points"""
    K, dist, f = camera(shift)
    obj = cc.prepare_object_points(BOARD, float(f["square"]))
    X = np.concatenate([obj, np.zeros((len(obj), 1))], axis=1)
    return lr.project_points(X, cc.rodrigues(f["rvecs"][view]), f["tvecs"][view], K, dist)[0]


def canonical(corners, board=BOARD):
    """rule 6's 180-degree convention applied to a row-major board: the first corner has the smaller (y, x)"""
    cols, rows = board
    a = np.asarray(corners, np.float64).reshape(rows, cols, 2)
    b = a[::-1, ::-1]
    return (b if (b[0, 0, 1], b[0, 0, 0]) < (a[0, 0, 1], a[0, 0, 0]) else a).reshape(rows * cols, 2)


@functools.lru_cache(maxsize=None)
def render(view, shift=(0.0, 0.0), size=SIZE):
    """-> uint8 [H, W] gray frame (read-only)"""
    K, dist, f = camera(shift)
    W, H = size
    R, t, sq = cc.rodrigues(f["rvecs"][view]), f["tvecs"][view].astype(np.float64), float(f["square"])
    cols, rows = BOARD
    edge = np.array([[u, v, 0.0] for u in (-2.0, cols + 1.0) for v in np.linspace(-2.0, rows + 1.0, 10)] +
                    [[u, v, 0.0] for v in (-2.0, rows + 1.0) for u in np.linspace(-2.0, cols + 1.0, 13)]) * sq
    px = lr.project_points(edge, R, t, K, dist)[0]
    xa, ya = np.maximum(np.floor(px.min(axis=0)).astype(int) - 4, 0)
    xb, yb = np.minimum(np.ceil(px.max(axis=0)).astype(int) + 5, (W, H))
    img = np.full((H, W), BACK, np.uint8)
    if xa >= xb or ya >= yb:
        return img
    off = (np.arange(SS) + 0.5) / SS - 0.5
    u = (np.arange(xa, xb)[:, None] + off[None, :]).reshape(-1)
    v = (np.arange(ya, yb)[:, None] + off[None, :]).reshape(-1)
    uu, vv = np.meshgrid(u, v)
    ray = lr.undistort_points(np.stack([uu, vv], -1), K, dist, iters=20, normalized=True)[0]
    d = np.stack([ray[..., 0], ray[..., 1], np.ones_like(uu)], -1)
    lam = (R[:, 2] @ t) / (d @ R[:, 2])                       # the ray meets the board's plane z_b = 0
    Xb = (lam[..., None] * d - t) @ R                         # R^T (lam d - t)
    bu, bv = Xb[..., 0] / sq, Xb[..., 1] / sq
    val = np.full(uu.shape, float(BACK))
    margin = (bu >= -2) & (bu < cols + 1) & (bv >= -2) & (bv < rows + 1) & (lam > 0) & np.isfinite(bu) & np.isfinite(bv)
    val[margin] = LIGHT
    inner = margin & (bu >= -1) & (bu < cols) & (bv >= -1) & (bv < rows)
    dark = inner & (((np.floor(bu) + np.floor(bv)).astype(np.int64) & 1) == 0)
    val[dark] = DARK
    val = val.reshape(yb - ya, SS, xb - xa, SS).mean(axis=(1, 3))
    img[ya:yb, xa:xb] = np.floor(val + 0.5).astype(np.uint8)
    img.setflags(write=False)
    return img


def channels(gray, ch):
    """a gray frame as ch channels that differ (B = g / 2, G = g, R = min(g + 20, 255), a fourth of 7), so that the weights
    matter"""
    if ch == 1:
        return np.ascontiguousarray(gray[..., None])
    planes = [gray // 2, gray, np.minimum(gray.astype(np.int64) + 20, 255).astype(np.uint8)] + ([np.full_like(gray, 7)] if ch == 4 else [])
    return np.ascontiguousarray(np.stack(planes, -1))


HALF_OUT_SHIFT = (-330.0, 0.0)   # view 0's board pushed over the frame's left edge
FLAT_POINT = [5.0, 5.0]          # background all round: the refinement's system is singular


def far_point(view=0, win=WIN):
    """a start one pixel more than the half window along x from the first corner: the refinement is drawn to the corner, ends
    farther from its start than the half window, and reverts (with the (11, 11) window only in view 13: in the smaller views
    another corner lies within 11 px of every start)"""
    return truth(view)[0] + [win[0] + 1.0, 0.0]


def border_case(view=0):
    """-> (the view cropped so that its first corner lies 2 px from the left edge, the start pixel, the corner's truth)"""
    t = truth(view)[0]
    x0 = int(np.rint(t[0])) - 2
    return np.ascontiguousarray(render(view)[:, x0:]), np.rint(t - [x0, 0.0]), t - [x0, 0.0]


@functools.lru_cache(maxsize=None)
def noise_frame(size=(193, 131), seed=7):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (size[1], size[0], 3), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def restated(view, shift=(0.0, 0.0), win=WIN):
    """the restatement's detection of a rendered view, computed once: (board or None, candidates, refined points, ok)"""
    return cs.find_chessboard_corners(render(view, shift), BOARD, win=win)
