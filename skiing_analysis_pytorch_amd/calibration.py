"""Camera calibration from chessboard corners and its ground-truth-free checks (camera_calibration/main.py), on top of the
device solver and the device lens model.

The solver (cv2.calibrateCamera in the reference) is `geometry.calibrate_camera` on the device: Zhang's start and a
Levenberg-Marquardt over the intrinsics and every board's pose, many view subsets in one call.  This module is the rest of
the reference's script without its pictures and files: the object points, the prune step, the reprojection and coverage
statistics, and the leave-one-out spread that a batch makes cheap.  Corners arrive as arrays, or are found in the frames:
`find_chessboard_corners` (the reference's findChessboardCorners + cornerSubPix step) runs `geometry.chessboard_candidates` and
`geometry.corner_subpix` on the device for all frames and orders each frame's points into the board with `order_chessboard`,
and `calibrate_from_frames` is the reference's flow from the pictures on.  The detector follows the project's own rules
(DESIGN §2 "Chessboard corners"), not OpenCV's quad-based one.  Sampling videos, reading pictures, getOptimalNewCameraMatrix /
valid_roi_fraction and stereo calibration are outside this build.  `formats.save_calibration` / `formats.load_calibration`
write and read the files.
Host module: small arrays, NumPy; the heavy steps run on the device.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Optional, Sequence, Tuple

import numpy as np


@dataclass
class CalibConfig:
    """The reference's CalibConfig without its picture, video and file fields, plus the frame size (the reference reads it
    off its first picture)."""
    board_cols: int = 9           # inner corners along columns
    board_rows: int = 6           # inner corners along rows
    square_size: float = 25.0     # same unit across all boards
    rational_model: bool = True   # frees k4 .. k6
    zero_tangent: bool = False    # holds p1 = p2 = 0
    prune_top_ratio: float = 0.1  # drop the worst share of the views once; 0 disables
    image_size: Optional[Tuple[int, int]] = None   # (width, height)
    max_evals: int = 200

    @property
    def board_size(self) -> Tuple[int, int]:
        return (self.board_cols, self.board_rows)

    @property
    def flags(self) -> int:
        """cv2's flags for the .yml: CALIB_RATIONAL_MODEL = 1 << 14, CALIB_ZERO_TANGENT_DIST = 1 << 3"""
        return (16384 if self.rational_model else 0) | (8 if self.zero_tangent else 0)


def prepare_object_points(board_size: Tuple[int, int], square_size: float) -> np.ndarray:
    """prepare_object_points (main.py:73-77): [cols * rows, 3] float32, x fastest, z = 0, scaled by the square's size."""
    cols, rows = board_size
    objp = np.zeros((cols * rows, 3), np.float32)
    objp[:, :2] = np.mgrid[0:cols, 0:rows].T.reshape(-1, 2)
    return objp * float(square_size)


def reproj_stats(err) -> Tuple[list, dict]:
    """compute_reproj_stats (main.py:154-167) from the solver's err [V, n] (NaN where unused; an all-NaN view is skipped):
    per view mean / median / 95th percentile, and the three over all corners together, with np.percentile's semantics."""
    err = np.asarray(err, np.float64)
    per_img, every = [], []
    for e in err:
        e = e[~np.isnan(e)]
        if e.size == 0:
            continue
        per_img.append({"mean_px": float(e.mean()), "median_px": float(np.median(e)), "p95_px": float(np.percentile(e, 95))})
        every.append(e)
    if not every:
        return per_img, {"global_mean_px": None, "global_median_px": None, "global_p95_px": None}
    cat = np.concatenate(every)
    return per_img, {"global_mean_px": float(cat.mean()), "global_median_px": float(np.median(cat)),
                     "global_p95_px": float(np.percentile(cat, 95))}


def convex_hull_area(points) -> float:
    """Area of the convex hull of points [N, 2] (cv2.convexHull + cv2.contourArea): Andrew's monotone chain, then the
    shoelace formula.  Fewer than 3 distinct points, or all collinear: 0."""
    pts = np.unique(np.asarray(points, np.float64).reshape(-1, 2), axis=0)     # sorted by x, then y
    if len(pts) < 3:
        return 0.0

    def chain(seq):
        out = []
        for q in seq:
            while len(out) >= 2 and ((out[-1][0] - out[-2][0]) * (q[1] - out[-2][1])
                                     - (out[-1][1] - out[-2][1]) * (q[0] - out[-2][0])) <= 0:
                out.pop()
            out.append(q)
        return out

    hull = np.array(chain(pts)[:-1] + chain(pts[::-1])[:-1])
    if len(hull) < 3:
        return 0.0
    x, y = hull[:, 0], hull[:, 1]
    return float(0.5 * abs(np.dot(x, np.roll(y, -1)) - np.dot(y, np.roll(x, -1))))


def edge_center_ratio(imgpoints: Sequence, image_size: Tuple[int, int], border_ratio: float = 0.2) -> dict:
    """compute_edge_center_ratio (main.py:170-189): the share of the w h frame that the convex hull of all corners covers,
    and the share of corners within border_ratio of a frame edge.  Non-finite corners are skipped; float64 throughout (the
    reference rounds the hull's input to float32)."""
    w, h = image_size
    pts = [np.asarray(p, np.float64).reshape(-1, 2) for p in imgpoints]
    if not pts:
        return {"coverage_ratio": 0.0, "edge_points_ratio": 0.0}
    pts = np.concatenate(pts)
    pts = pts[np.isfinite(pts).all(axis=1)]
    if len(pts) == 0:
        return {"coverage_ratio": 0.0, "edge_points_ratio": 0.0}
    xs, ys = pts[:, 0], pts[:, 1]
    at_edge = ((xs < w * border_ratio) | (xs > w * (1 - border_ratio)) | (ys < h * border_ratio) | (ys > h * (1 - border_ratio))).mean()
    return {"coverage_ratio": float(convex_hull_area(pts) / (w * h)), "edge_points_ratio": float(at_edge)}


def prune_mask(mean_err, prune_top_ratio: float) -> Optional[np.ndarray]:
    """The reference's prune rule (main.py:303-308) on the per-view mean errors: with prune_top_ratio > 0 and >= 20 views, the
    views whose mean exceeds the 1 - ratio quantile are dropped, provided some are and >= 10 remain -> the keep mask, or None
    when nothing is to be pruned."""
    means = np.asarray(mean_err, np.float64)
    if not (prune_top_ratio > 0 and len(means) >= 20):
        return None
    keep = means <= np.quantile(means, 1 - prune_top_ratio)
    if (~keep).sum() == 0 or keep.sum() < 10:
        return None
    return keep


def fov_and_principal(K, image_size: Tuple[int, int]) -> dict:
    """compute_fov_and_principal (main.py:192-207): focal lengths, principal point, the horizontal / vertical field of view
    of a (width, height) frame in degrees, the principal point's offset from the frame centre, and fx / fy."""
    K = np.asarray(K, np.float64)
    w, h = image_size
    fx, fy, cx, cy = float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])
    return {"fx": fx, "fy": fy, "cx": cx, "cy": cy,
            "hfov_deg": float(2 * np.degrees(np.arctan(w / (2 * fx)))),
            "vfov_deg": float(2 * np.degrees(np.arctan(h / (2 * fy)))),
            "principal_point_offset_px": (cx - w / 2, cy - h / 2),
            "aspect_fx_fy": (fx / fy) if fy else None}


def line_fit_rms(points, cols: int, rows: int) -> float:
    """points [boards * rows * cols, 2], every board row-major with `cols` corners a row -> sqrt of the mean, over every board
    row and column, of the mean squared distance of its corners to their least-squares line y = m x + c."""
    errs = []
    for board in np.asarray(points, np.float64).reshape(-1, rows * cols, 2):
        lines = [board[r * cols:(r + 1) * cols] for r in range(rows)] + [board[c::cols] for c in range(cols)]
        for pts in lines:
            x, y = pts[:, 0], pts[:, 1]
            m, c = np.linalg.lstsq(np.stack([x, np.ones_like(x)], 1), y, rcond=None)[0]
            d = np.abs(m * x - y + c) / np.sqrt(m * m + 1)
            errs.append(np.mean(d * d))
    return float(np.sqrt(np.mean(errs))) if errs else float("nan")


def _undistort_on_device(x: np.ndarray, K, dist) -> np.ndarray:
    import torch

    from . import geometry
    return geometry.undistort_points(torch.from_numpy(x).cuda(), K, dist).x.cpu().numpy()


def line_straightness(imgpoints: Sequence, board_size: Tuple[int, int], K, dist,
                      undistort: Optional[Callable] = None) -> dict:
    """line_straightness_on_corners (main.py:210-237): a chessboard's rows and columns are straight in the world, so they are
    straight in an ideal pinhole image.  imgpoints: the detected corners of every board, each [rows * cols, 2] (or cv2's
    [rows * cols, 1, 2]) row-major; board_size = (cols, rows) -> the RMS line-fit error in pixels of the corners as detected
    and after undistortPoints(x, K, dist, P=K).  A good calibration takes the second figure to the detector's noise.
    undistort: a function (x float64 [N, 2], K, dist) -> [N, 2] to use in place of geometry.undistort_points, which needs the
    device.  The corners stay float64 (the reference rounds them to float32 first)."""
    cols, rows = board_size
    pts = np.concatenate([np.asarray(p, np.float64).reshape(-1, 2) for p in imgpoints], axis=0)
    und = np.asarray((undistort or _undistort_on_device)(np.ascontiguousarray(pts), K, dist), np.float64)
    return {"straightness_rms_before_px": line_fit_rms(pts, cols, rows),
            "straightness_rms_after_px": line_fit_rms(und, cols, rows)}


def _solve(corners, cfg: CalibConfig, image_size, use=None):
    """corners [V, n, 2] -> geometry.calibrate_camera's result as NumPy arrays (one read-back, after the call)"""
    import torch

    from . import geometry
    size = image_size or cfg.image_size
    if size is None:
        raise ValueError("calibration needs the frame's (width, height): image_size, or CalibConfig.image_size")
    img = np.ascontiguousarray(np.asarray(corners, np.float64).reshape(len(corners), -1, 2))
    obj = prepare_object_points(cfg.board_size, cfg.square_size)[:, :2].astype(np.float64)
    if img.shape[1] != obj.shape[0]:
        raise ValueError(f"every board needs {obj.shape[0]} corners ({cfg.board_cols} x {cfg.board_rows}), got {img.shape[1]}")
    r = geometry.calibrate_camera(torch.from_numpy(obj).cuda(), torch.from_numpy(img).cuda(), size,
                                  use=None if use is None else torch.from_numpy(np.ascontiguousarray(use, dtype=np.uint8)).cuda(),
                                  rational_model=cfg.rational_model, zero_tangent=cfg.zero_tangent, max_evals=cfg.max_evals)
    return img, tuple(int(x) for x in size), {k: getattr(r, k).cpu().numpy() for k in r._fields}


def calibrate_camera(corners, cfg: CalibConfig, image_size: Optional[Tuple[int, int]] = None, names: Optional[Sequence[str]] = None,
                     undistort: Optional[Callable] = None) -> dict:
    """calibrate_camera (main.py:250-380) from detected corners: corners [V, n, 2] (or cv2's [V, n, 1, 2]), every board
    row-major with cfg.board_cols corners a row; names: one per view (default view_0000 ..) -> the reference's result dict
    (status, rms_reproj_error, camera_matrix, dist_coeffs, num_images, image_size, used_names, dropped_names, the global
    reprojection, coverage, field-of-view and straightness figures; the last over the boards with every corner finite), without per_image_csv and the valid-ROI figures, plus
    rvecs, tvecs [num_images, 3], per_image (the CSV's rows), std_intrinsics (geometry.CALIB_PARAMS' order) and
    rms_before_prune.  The prune step is the reference's: the second calibration runs through the solver's `use` mask and is
    accepted iff its rms fell.  dist_coeffs holds 5 coefficients, or 8 with the rational model."""
    img, size, r = _solve(corners, cfg, image_size)
    V = img.shape[0]
    names = [f"view_{i:04d}" for i in range(V)] if names is None else list(names)
    if len(names) != V:
        raise ValueError(f"{len(names)} names for {V} views")
    if not np.isfinite(r["rms"][0]):
        return {"status": "Failed", "reason": "fewer than 3 usable views", "num_images": int(r["n_views"][0])}
    used = ~np.isnan(r["mean_err"][0])
    rms_first = float(r["rms"][0])
    dropped = []
    keep = prune_mask(r["mean_err"][0][used], cfg.prune_top_ratio)
    if keep is not None:
        idx = np.flatnonzero(used)
        use = np.zeros((1, V), np.uint8)
        use[0, idx[keep]] = 1
        _, _, r2 = _solve(corners, cfg, size, use=use)
        if r2["rms"][0] < r["rms"][0]:                     # accept iff the rms fell (a NaN fails)
            dropped = [names[i] for i in idx[~keep]]
            r, used = r2, ~np.isnan(r2["mean_err"][0])
    K, n_coef = r["K"][0], 8 if cfg.rational_model else 5
    dist = r["dist"][0][:n_coef].copy()
    per_img, global_stats = reproj_stats(r["err"][0])
    kept = [names[i] for i in np.flatnonzero(used)]
    for row, name in zip(per_img, kept):
        row["image_name"] = name
    return {"status": "Success", "rms_reproj_error": float(r["rms"][0]), "camera_matrix": K, "dist_coeffs": dist,
            "num_images": len(kept), "image_size": size, "used_names": kept, "dropped_names": dropped, **global_stats,
            **edge_center_ratio(img[used], size, border_ratio=0.2), **fov_and_principal(K, size),
            **line_straightness(img[used & np.isfinite(img).all(axis=(1, 2))], cfg.board_size, K, dist, undistort=undistort),
            "rvecs": r["rvec"][0][used], "tvecs": r["t"][0][used], "per_image": per_img, "std_intrinsics": r["std"][0],
            "rms_before_prune": rms_first, "n_evals": int(r["n_evals"][0]), "converged": bool(r["success"][0])}


# ---- chessboard corners from frames: the device detector's candidates ordered into a board (DESIGN §2 "Chessboard corners") ----
_GRID_STEPS = ((1, 0), (-1, 0), (0, 1), (0, -1))


def _grow_grid(pts: np.ndarray, D: np.ndarray, seed: int, limit: int) -> Optional[dict]:
    """rule 6's growth from one seed -> {(i, j): point index}, or None when the seed has no two usable first steps or the grid
    outgrows `limit` cells a side"""
    j1 = int(np.argmin(D[seed]))
    l1 = D[seed, j1]
    if not np.isfinite(l1) or l1 <= 0:
        return None
    e1 = pts[j1] - pts[seed]
    j2 = None
    for j in np.argsort(D[seed], kind="stable"):
        lj = D[seed, j]
        if not np.isfinite(lj) or lj > 2.0 * l1:
            break
        if j == j1 or lj < 0.5 * l1:
            continue
        if abs(float(np.dot(pts[j] - pts[seed], e1))) / (lj * l1) < 0.6:
            j2 = int(j)
            break
    if j2 is None:
        return None
    cells = {(0, 0): seed, (1, 0): j1, (0, 1): j2}
    free = np.ones(len(pts), bool)
    free[[seed, j1, j2]] = False
    queue = [(0, 0), (1, 0), (0, 1)]
    head = 0
    while head < len(queue):                      # breadth-first; a filled cell sends its filled neighbours round again
        c = queue[head]
        head += 1
        P = pts[cells[c]]
        for d in _GRID_STEPS:
            t = (c[0] + d[0], c[1] + d[1])
            if t in cells:
                continue
            back = (c[0] - d[0], c[1] - d[1])
            step = None
            if back in cells:
                step = P - pts[cells[back]]
            else:                                 # no cell behind: the parallel edge of an adjacent row
                for e in ((d[1], d[0]), (-d[1], -d[0])):
                    a, b = (c[0] + e[0], c[1] + e[1]), (t[0] + e[0], t[1] + e[1])
                    if a in cells and b in cells:
                        step = pts[cells[b]] - pts[cells[a]]
                        break
            if step is None:
                continue
            dist = np.hypot(*(pts - (P + step)).T)
            dist[~free] = np.inf
            k = int(np.argmin(dist))
            if not dist[k] <= 0.35 * float(np.hypot(*step)):
                continue
            cells[t] = k
            free[k] = False
            ii, jj = [q[0] for q in cells], [q[1] for q in cells]
            if max(ii) - min(ii) >= limit or max(jj) - min(jj) >= limit:
                return None
            queue.append(t)
            queue.extend(q for q in ((t[0] + s[0], t[1] + s[1]) for s in _GRID_STEPS) if q in cells)
    return cells


def _normalise_grid(pts: np.ndarray, cells: dict, cols: int, rows: int) -> Optional[np.ndarray]:
    """a grown grid -> [rows, cols, 2] under rule 6's normalisation, or None unless it is complete and exactly the board"""
    i0, j0 = min(q[0] for q in cells), min(q[1] for q in cells)
    ni, nj = max(q[0] for q in cells) - i0 + 1, max(q[1] for q in cells) - j0 + 1
    if len(cells) != cols * rows or ni * nj != len(cells):
        return None
    if (ni, nj) == (cols, rows):
        arr = np.array([[pts[cells[(i0 + c, j0 + r)]] for c in range(cols)] for r in range(rows)])
    elif (ni, nj) == (rows, cols):
        arr = np.array([[pts[cells[(i0 + r, j0 + c)]] for c in range(cols)] for r in range(rows)])
    else:
        return None
    col, row = arr[0, 1] - arr[0, 0], arr[1, 0] - arr[0, 0]
    if col[0] * row[1] - col[1] * row[0] <= 0:    # a mirrored board: the columns run the other way
        arr = arr[:, ::-1]
    other = arr[::-1, ::-1]                       # the same board turned by 180 degrees
    if (other[0, 0, 1], other[0, 0, 0]) < (arr[0, 0, 1], arr[0, 0, 0]):
        arr = other
    return np.ascontiguousarray(arr)


def order_chessboard(points, board_size: Tuple[int, int], strength=None) -> Optional[np.ndarray]:
    """The refined candidates of one frame -> the board's corners [cols * rows, 2], row-major like prepare_object_points, or
    None.  points [m, 2] pixels (non-finite rows are skipped), board_size = (cols, rows) with both >= 2, strength [m]
    (default: the input order, strongest first).  A point within 1 px of a stronger one is dropped.  Seeds are tried in
    descending strength: the first step goes to the seed's nearest neighbour, the second to the nearest neighbour whose
    length is within [0.5, 2] x the first and whose |cos| against it is < 0.6; the grid then grows breadth-first, a cell
    predicted as 2 P - P_back (or P + the parallel edge of the adjacent row when there is no cell behind) taking the
    nearest unused point within 0.35 x the predicted step.  A grid is accepted only if it is complete and exactly cols x
    rows (or its transpose): distractors beside the board are left out, a missing corner or a point that continues the
    grid gives None.  The columns run along `cols`, cross(column step, row step) > 0 in image coordinates (no mirrored
    board), and of the two remaining boards, 180 degrees apart, the first corner is the one with the smaller (y, x)."""
    cols, rows = (int(v) for v in board_size)
    if cols < 2 or rows < 2:
        raise ValueError(f"order_chessboard: the board needs at least 2 x 2 inner corners, got {cols} x {rows}")
    pts = np.asarray(points, np.float64).reshape(-1, 2)
    s = -np.arange(len(pts), dtype=np.float64) if strength is None else np.asarray(strength, np.float64).reshape(-1)
    if len(s) != len(pts):
        raise ValueError(f"order_chessboard: {len(s)} strengths for {len(pts)} points")
    good = np.isfinite(pts).all(axis=1) & ~np.isnan(s)
    pts, s = pts[good], s[good]
    pts = pts[np.argsort(-s, kind="stable")]
    keep = []
    for i, p in enumerate(pts):
        if not keep or np.hypot(*(pts[keep] - p).T).min() > 1.0:
            keep.append(i)
    pts = pts[keep]
    if len(pts) < cols * rows:
        return None
    D = np.hypot(pts[:, None, 0] - pts[None, :, 0], pts[:, None, 1] - pts[None, :, 1])
    np.fill_diagonal(D, np.inf)
    for seed in range(len(pts)):
        cells = _grow_grid(pts, D, seed, max(cols, rows))
        arr = None if cells is None else _normalise_grid(pts, cells, cols, rows)
        if arr is not None:
            return arr.reshape(cols * rows, 2)
    return None


def find_chessboard_corners(frames, board_size: Tuple[int, int], win: Tuple[int, int] = (11, 11), threshold: int = 38,
                            nms_radius: int = 4, max_candidates: int = 1024, iters: int = 30) -> Tuple[np.ndarray, np.ndarray]:
    """find_chessboard_corners (main.py:80-90) for every frame at once: frames uint8 [F, H, W, ch] or [C, F, H, W, ch] on the
    device (colour channels in cv2's B, G, R order) -> corners float64 [..., cols * rows, 2] (NaN rows where no board was
    found) and found bool [...].  geometry.chessboard_candidates and geometry.corner_subpix run on the device for all frames,
    one read-back brings the candidates over, order_chessboard orders each frame's on the host.  win is cornerSubPix's half
    window: the reference's (11, 11) suits boards whose squares are wider than the window; take (5, 5) for small boards."""
    import torch

    from . import geometry
    cols, rows = (int(v) for v in board_size)
    cand = geometry.chessboard_candidates(frames, threshold=threshold, nms_radius=nms_radius, max_candidates=max_candidates)
    ref = geometry.corner_subpix(frames, cand.xy, cand.count, win=win, iters=iters)
    lead, M = tuple(cand.count.shape), int(cand.xy.shape[-2])
    N = int(np.prod(lead, dtype=np.int64))
    back = torch.cat([ref.points.reshape(N, 2 * M), ref.ok.reshape(N, M).double(), cand.response.reshape(N, M).double(),
                      cand.count.reshape(N, 1).double()], dim=1).cpu().numpy()           # the one read-back
    pts, ok, resp, count = back[:, :2 * M].reshape(N, M, 2), back[:, 2 * M:3 * M] != 0, back[:, 3 * M:4 * M], back[:, 4 * M]
    corners, found = np.full((N, cols * rows, 2), np.nan), np.zeros(N, bool)
    for f in range(N):
        sel = ok[f] & (np.arange(M) < count[f])
        board = order_chessboard(pts[f][sel], (cols, rows), strength=resp[f][sel])
        if board is not None:
            corners[f], found[f] = board, True
    return corners.reshape(lead + (cols * rows, 2)), found.reshape(lead)


def calibrate_from_frames(frames, cfg: CalibConfig, names: Optional[Sequence[str]] = None, win: Tuple[int, int] = (11, 11),
                          undistort: Optional[Callable] = None) -> dict:
    """calibrate_camera (main.py:250-323) from the pictures themselves: frames uint8 [F, H, W, ch] (or [C, F, H, W, ch], taken as
    C F pictures of one camera) on the device; names: one per frame (default view_0000 ..).  The boards are detected
    (find_chessboard_corners), frames without one are dropped, and calibrate_camera runs on the rest with the frames' own
    (width, height) -> its result plus num_detected; used_names are the names of the frames that went into the result.  No
    board in any frame: the reference's {"status": "Failed", "reason": "No corners detected", "num_images": 0}."""
    corners, found = find_chessboard_corners(frames, cfg.board_size, win=win)
    corners, found = corners.reshape(-1, corners.shape[-2], 2), found.reshape(-1)
    names = [f"view_{i:04d}" for i in range(len(found))] if names is None else list(names)
    if len(names) != len(found):
        raise ValueError(f"{len(names)} names for {len(found)} frames")
    if not found.any():
        return {"status": "Failed", "reason": "No corners detected", "num_images": 0}
    size = (int(frames.shape[-2]), int(frames.shape[-3]))
    result = calibrate_camera(corners[found], cfg, image_size=size, names=[names[i] for i in np.flatnonzero(found)],
                              undistort=undistort)
    result["num_detected"] = int(found.sum())
    return result


def leave_one_out(corners, cfg: CalibConfig, image_size: Optional[Tuple[int, int]] = None) -> dict:
    """The V calibrations that each leave one view out, in one device call (group v omits view v) -> K [V, 3, 3], dist [V, 12],
    rms [V], success [V] and spread: per parameter (geometry.CALIB_PARAMS' order) the mean, std, min and max over the
    groups that succeeded in stopping on a finite result.  A parameter whose spread is large against its std_intrinsics
    depends on single views."""
    from . import geometry
    V = len(corners)
    _, _, r = _solve(corners, cfg, image_size, use=1 - np.eye(V, dtype=np.uint8))
    p = np.concatenate([r["K"][:, [0, 1, 0, 1], [0, 1, 2, 2]], r["dist"][:, :8]], axis=1)
    ok = np.isfinite(p).all(axis=1)
    q = p[ok] if ok.any() else np.full((1, 12), np.nan)
    return {"K": r["K"], "dist": r["dist"], "rms": r["rms"], "success": r["success"], "n_evals": r["n_evals"],
            "spread": {"names": list(geometry.CALIB_PARAMS), "mean": q.mean(axis=0), "std": q.std(axis=0), "min": q.min(axis=0),
                       "max": q.max(axis=0)}}
