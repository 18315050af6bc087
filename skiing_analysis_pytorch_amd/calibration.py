"""Ground-truth-free checks of a camera calibration (camera_calibration/main.py:192-237), on top of the device lens model.

The calibration solver itself (cv2.calibrateCamera) is outside this build; what a calibration file holds is read by
`formats.load_calibration`.  Host module: small arrays, NumPy; the one heavy step, undistorting the detected corners, is
`geometry.undistort_points` on the device.
"""
from __future__ import annotations

from typing import Callable, Optional, Sequence, Tuple

import numpy as np


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
