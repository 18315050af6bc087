"""Lens distortion of points (csrc/lens.hip; C-ABI: skimi_distort_points, skimi_undistort_points, skimi_project_points; the
frames' skimi_undistort_u8 is bound in preprocess.py): camera_calibration/calibration_parameters.* +
triangulation/postprocess.py:89-97, from OpenCV's documented model; rules: include/skimi.h, DESIGN §2 "Lens distortion".

OpenCV's rational + tangential + thin-prism model.  Calibrations are small HOST arrays (NumPy, lists or CPU tensors; a
device tensor is copied back): they reach the kernels by value.  Batch rule of the three point functions: K [3, 3] is
one camera for every point of x [..., 2]; K [C, 3, 3] is one camera per entry of the axis before the points' own,
x [..., C, n, 2], and everything in front of that axis is batch (keypoints [T, V, J, 2] with a calibration per view:
one launch).  dist is [k] (shared) or [C, k], k in LENS_COEFF_COUNTS.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch

from .._args import camera_matrices, contig_as, f64, host_f64, host_ptr, on_device, per_camera_coeffs
from .._lib import SkimiError, check, current_stream, lib, ptr

LENS_MAX_CAMERAS, LENS_MAX_ITERS = 8, 1000
LENS_COEFF_COUNTS = (4, 5, 8, 12, 14)


class UndistortResult(NamedTuple):
    """undistort_points' outputs (float64 device tensors unless the call was the identity)."""
    x: torch.Tensor          # [..., 2]: undistorted points, pixels of P (default K) or normalised coordinates
    resid_px: torch.Tensor   # [...]: pixel distance between the input and the re-distorted result; NaN with a NaN point


class ProjectResult(NamedTuple):
    """project_points' outputs (float64 device tensors)."""
    x: torch.Tensor          # [..., 2]: pixels of K
    depth: torch.Tensor      # [...]: z in the camera frame


def lens_coeffs(dist) -> np.ndarray:
    """OpenCV coefficient vectors [..., k], k = 4, 5, 8, 12 or 14 in cv2's order (k1 k2 p1 p2 k3 k4 k5 k6 s1 s2 s3 s4 tx ty) ->
    float64 [..., 12], zero-padded.  None: twelve zeros.  Non-zero tx / ty (the tilt model) is refused."""
    if dist is None:
        return np.zeros(12, np.float64)
    d = host_f64(dist)
    if d.ndim == 2 and d.shape[0] == 1 and d.shape[1] in LENS_COEFF_COUNTS:
        d = d[0]                     # cv2 hands its vectors out as [1, k]
    if d.ndim < 1 or d.shape[-1] not in LENS_COEFF_COUNTS:
        raise ValueError(f"distortion coefficients must come as 4, 5, 8, 12 or 14 numbers, got shape {list(d.shape)}")
    if d.shape[-1] == 14:
        if np.any(d[..., 12:] != 0):
            raise ValueError("the tilt model (non-zero tx, ty) is not supported")
        d = d[..., :12]
    if not np.isfinite(d).all():
        raise ValueError("distortion coefficients must be finite")
    out = np.zeros(d.shape[:-1] + (12,), np.float64)
    out[..., :d.shape[-1]] = d
    return out


def _lens_setup(name, x, K, dist, last):
    """-> (K [C, 3, 3], dist [C, 12], per_camera, outer, C, n) for points x [..., last] under the batch rule above"""
    on_device(name, x, what="a device tensor of points")
    if x.dim() < 1 or x.shape[-1] != last:
        raise ValueError(f"{name}: points must be [..., {last}], got {list(x.shape)}")
    per_camera = host_f64(K).ndim == 3
    Kh = camera_matrices(name, "K", K, None)
    C = Kh.shape[0]
    if C > LENS_MAX_CAMERAS:
        raise ValueError(f"{name}: at most {LENS_MAX_CAMERAS} cameras a call, got {C}")
    d = per_camera_coeffs(name, lens_coeffs(dist), C)
    if per_camera:
        if x.dim() < 3 or x.shape[-3] != C:
            raise ValueError(f"{name}: K holds {C} cameras, so points must be [..., {C}, n, {last}], got {list(x.shape)}")
        outer, n = int(np.prod(x.shape[:-3], dtype=np.int64)), int(x.shape[-2])
    else:
        outer, n = 1, int(np.prod(x.shape[:-1], dtype=np.int64))
    return Kh, d, per_camera, outer, C, n


def _identity(normalized, d, Ph, Kh):
    """all-zero coefficients with P equal to K and pixels on both sides: the lens changes nothing"""
    return not normalized and not d.any() and (Ph is None or np.array_equal(Ph, Kh))


def distort_points(x: torch.Tensor, K, dist, P=None, normalized: bool = False) -> torch.Tensor:
    """Undistorted points -> where the real lens images them, in one launch: x [..., 2] device tensor, as pixels of P
    (default K) or, normalized=True, as normalised coordinates -> float64 pixels of K.  The exact inverse direction of
    undistort_points with the same arguments.  All-zero coefficients with P equal to K and pixels in: the input object is
    returned unchanged."""
    Kh, d, _pc, outer, C, n = _lens_setup("distort_points", x, K, dist, 2)
    Ph = None if P is None else camera_matrices("distort_points", "P", P, C)
    if _identity(normalized, d, Ph, Kh):
        return x
    xi = contig_as(x, torch.float64)
    out = torch.empty_like(xi)
    check(lib().skimi_distort_points(ptr(xi), host_ptr(Kh), host_ptr(d), host_ptr(Ph), None, outer, C, n, 1 if normalized else 0,
                                     ptr(out), current_stream()), "skimi_distort_points")
    return out


def undistort_points(x: torch.Tensor, K, dist, P=None, iters: int = 20, normalized: bool = False) -> UndistortResult:
    """cv2.undistortPoints(x, K, dist, P=P) in one launch: distorted pixels x [..., 2] (device) of K -> UndistortResult(x,
    resid_px), the points as pixels of P (default K) or, normalized=True, as normalised coordinates (cv2's result without
    P).  OpenCV's fixed-point iteration with exactly `iters` rounds (cv2 runs 5; no early exit: bitwise reproducible).
    resid_px is the pixel distance between the input and the re-distorted result: it exposes a point that did not converge
    or lies beyond the model's invertible range.  A NaN keypoint gives NaN in its own row only.  All-zero coefficients
    with P equal to K and pixels out: the input object is returned unchanged, with a zero residual."""
    Kh, d, _pc, outer, C, n = _lens_setup("undistort_points", x, K, dist, 2)
    Ph = None if P is None else camera_matrices("undistort_points", "P", P, C)
    iters = int(iters)
    if not 0 <= iters <= LENS_MAX_ITERS:
        raise ValueError(f"undistort_points: iters must be in 0..{LENS_MAX_ITERS}, got {iters}")
    if _identity(normalized, d, Ph, Kh):
        return UndistortResult(x, torch.zeros(x.shape[:-1], dtype=torch.float64, device=x.device))
    xi = contig_as(x, torch.float64)
    out, resid = torch.empty_like(xi), f64(xi.device, *xi.shape[:-1])
    check(lib().skimi_undistort_points(ptr(xi), host_ptr(Kh), host_ptr(d), host_ptr(Ph), None, outer, C, n, iters,
                                       1 if normalized else 0, ptr(out), ptr(resid), current_stream()), "skimi_undistort_points")
    return UndistortResult(out, resid)


def undistort_keypoints_steps(keypoints: torch.Tensor, K: torch.Tensor, dist, iters: int = 20) -> UndistortResult:
    """post_triage_single's rule, undistortPoints(x, K, d, P=K), for keypoints [T, V, J, 2] whose K [T, V, 3, 3] is a DEVICE
    tensor with one matrix per step and view (the model's own intrinsics): the kernel reads K from memory, the per-view
    coefficients dist ([k] or [V, k]) travel by value.  One launch; float64 out."""
    if keypoints.dim() != 4 or keypoints.shape[-1] != 2 or tuple(K.shape) != tuple(keypoints.shape[:2]) + (3, 3):
        raise ValueError(f"undistort_keypoints_steps: need keypoints [T, V, J, 2] and K [T, V, 3, 3], got {list(keypoints.shape)}, "
                         f"{list(K.shape)}")
    if not keypoints.is_cuda or K.device != keypoints.device:
        raise SkimiError("undistort_keypoints_steps needs keypoints and K on one device")
    T, V, J, _ = keypoints.shape
    if V > LENS_MAX_CAMERAS:
        raise ValueError(f"undistort_keypoints_steps: at most {LENS_MAX_CAMERAS} views, got {V}")
    d = per_camera_coeffs("undistort_keypoints_steps", lens_coeffs(dist), V)
    xi, Kd = contig_as(keypoints, torch.float64), contig_as(K, torch.float64)
    out, resid = torch.empty_like(xi), f64(xi.device, T, V, J)
    check(lib().skimi_undistort_points(ptr(xi), None, host_ptr(d), None, ptr(Kd), T, V, J, int(iters), 0, ptr(out), ptr(resid),
                                       current_stream()), "skimi_undistort_points")
    return UndistortResult(out, resid)


def _undistorted_f32(keypoints, K, dist):
    """the keypoints the triangulations see under dist=: unchanged (the same object) for None or all-zero coefficients"""
    if dist is None or not lens_coeffs(dist).any():
        return keypoints
    return undistort_keypoints_steps(keypoints, K, dist).x.to(torch.float32)


def project_points(X: torch.Tensor, R, t, K, dist=None) -> ProjectResult:
    """cv2.projectPoints with rotation matrices in place of rvec, in one launch: X [..., 3] device tensor in the world frame,
    R [3, 3] / t [3] (or [C, 3, 3] / [C, 3] with K [C, 3, 3] and X [..., C, n, 3]) host arrays, dist None or coefficients ->
    ProjectResult(x float64 [..., 2] pixels of K, depth float64 [...] = z in the camera frame).  Points behind the camera
    are projected as the formula says, as cv2 does."""
    Kh, d, per_camera, outer, C, n = _lens_setup("project_points", X, K, dist, 3)
    Rh, th = host_f64(R), host_f64(t)
    if tuple(Rh.shape) != ((C, 3, 3) if per_camera else (3, 3)) or tuple(th.shape) != ((C, 3) if per_camera else (3,)):
        raise ValueError(f"project_points: R / t must match K ({'[C, 3, 3] / [C, 3]' if per_camera else '[3, 3] / [3]'}), got "
                         f"{list(Rh.shape)}, {list(th.shape)}")
    if not (np.isfinite(Rh).all() and np.isfinite(th).all()):
        raise ValueError("project_points: R and t must be finite")
    Xi = contig_as(X, torch.float64)
    px, depth = f64(Xi.device, *Xi.shape[:-1], 2), f64(Xi.device, *Xi.shape[:-1])
    check(lib().skimi_project_points(ptr(Xi), host_ptr(Rh), host_ptr(th), host_ptr(Kh), host_ptr(d), outer, C, n, ptr(px), ptr(depth),
                                     current_stream()), "skimi_project_points")
    return ProjectResult(px, depth)
