"""Camera calibration from chessboard corners: Zhang's start + Levenberg-Marquardt (csrc/calibrate.hip; C-ABI:
skimi_calibrate_workspace_bytes, skimi_calibrate_camera): camera_calibration/main.py; the reference's names are the
package's calibration.py; rules: DESIGN §2 "Calibration".
"""
from __future__ import annotations

from typing import NamedTuple

import torch

from .._args import add_lead, f64, i32, on_device, to_dev, workspace
from .._lib import check, current_stream, lib, ptr

CALIB_PARAMS = ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3", "k4", "k5", "k6")   # the order of free_mask and std


class CalibrationResult(NamedTuple):
    """calibrate_camera's outputs (device tensors; G groups, V views, n corners a board)."""
    K: torch.Tensor          # float64 [G, 3, 3]; NaN for a failed group
    dist: torch.Tensor       # float64 [G, 12]: k1 k2 p1 p2 k3 k4 k5 k6 0 0 0 0, the lens block's order
    R: torch.Tensor          # float64 [G, V, 3, 3]; NaN for an unused view
    t: torch.Tensor          # float64 [G, V, 3]
    rvec: torch.Tensor       # float64 [G, V, 3]: cv2.Rodrigues(R)
    err: torch.Tensor        # float64 [G, V, n]: pixel distance, NaN where unused
    mean_err: torch.Tensor   # float64 [G, V]
    rms_err: torch.Tensor    # float64 [G, V]
    max_err: torch.Tensor    # float64 [G, V]
    rms: torch.Tensor        # float64 [G]: sqrt(cost / used corners), cv2.calibrateCamera's return value
    cost0: torch.Tensor      # float64 [G]: sum r^2 at the start
    cost: torch.Tensor       # float64 [G]
    std: torch.Tensor        # float64 [G, 12]: standard deviations in CALIB_PARAMS' order, NaN for a fixed parameter
    n_evals: torch.Tensor    # int32 [G]: cost evaluations, the start's included
    n_views: torch.Tensor    # int32 [G]: used views
    n_corners: torch.Tensor  # int32 [G]: used corners of the used views
    success: torch.Tensor    # bool [G]: stopped on the step criterion


def calib_free_mask(free=None, rational_model: bool = True, zero_tangent: bool = False) -> int:
    """The 12-bit mask of free intrinsics: the reference's switches (rational_model False: fx fy cx cy k1 k2 p1 p2 k3; True:
    k4 k5 k6 as well; zero_tangent clears p1 p2), or an explicit tuple of names from CALIB_PARAMS."""
    if free is None:
        free = ["fx", "fy", "cx", "cy", "k1", "k2", "k3"] + (["k4", "k5", "k6"] if rational_model else [])
        free += [] if zero_tangent else ["p1", "p2"]
    unknown = [k for k in free if k not in CALIB_PARAMS]
    if unknown:
        raise ValueError(f"calibrate_camera: unknown parameter {unknown[0]!r}; known: {list(CALIB_PARAMS)}")
    return sum(1 << CALIB_PARAMS.index(k) for k in set(free))


def calibrate_camera(obj: torch.Tensor, img: torch.Tensor, image_size, use=None, K0=None, dist0=None, free=None,
                     rational_model: bool = True, zero_tangent: bool = False, max_evals: int = 200) -> CalibrationResult:
    """cv2.calibrateCamera on the corners of a plane target, for G view subsets in one call: obj [n, 2] (the board's corners in
    its plane, shared by all boards), img [V, n, 2] pixels (a corner with a non-finite coordinate is skipped), image_size =
    (width, height), use [G, V] bool / uint8 or None (one group with every view), K0 [G, 3, 3] (or [3, 3]) and dist0 [G, k]
    (or [k], k <= 12 in OpenCV's order) or None -> CalibrationResult.  free: a tuple of names from CALIB_PARAMS, or None for
    the reference's switches rational_model / zero_tangent.  Zhang's start from the boards' homographies, then Levenberg-
    Marquardt with Marquardt's scaling over the free intrinsics and every used view's pose, the step solved through the
    Schur complement on the views; std from the same complement.  A group with fewer than 3 usable views is NaN with success
    False.  Nothing is read back.  Rules: DESIGN §2 "Calibration"."""
    on_device("calibrate_camera", obj, img, use, K0, dist0)
    if obj.dim() != 2 or obj.shape[1] != 2 or img.dim() != 3 or img.shape[1:] != (obj.shape[0], 2):
        raise ValueError(f"calibrate_camera: need obj [n, 2] and img [V, n, 2], got {list(obj.shape)}, {list(img.shape)}")
    mask = calib_free_mask(free, rational_model, zero_tangent)
    width, height = (int(x) for x in image_size)
    dev = obj.device
    V, n = int(img.shape[0]), int(img.shape[1])
    if K0 is not None:
        K0 = add_lead(K0, 3)[0]
    if dist0 is not None:
        dist0 = add_lead(dist0, 2)[0]
    sizes = [int(a.shape[0]) for a in (use, K0, dist0) if a is not None]
    G = sizes[0] if sizes else 1
    if use is not None and (use.dim() != 2 or use.shape[1] != V):
        raise ValueError(f"calibrate_camera: use must be [G, {V}], got {list(use.shape)}")
    if K0 is not None and tuple(K0.shape[1:]) != (3, 3):
        raise ValueError(f"calibrate_camera: K0 must be [G, 3, 3], got {list(K0.shape)}")
    if dist0 is not None and (dist0.dim() != 2 or dist0.shape[1] > 12):
        raise ValueError(f"calibrate_camera: dist0 must be [G, k <= 12], got {list(dist0.shape)}")
    if any(g != G for g in sizes):
        raise ValueError(f"calibrate_camera: use, K0 and dist0 disagree on the number of groups: {sizes}")
    obj, img = to_dev(obj, dev=dev), to_dev(img, dev=dev)
    if use is not None:
        use = to_dev(use != 0, torch.uint8, dev)
    K0 = to_dev(K0, dev=dev)
    if dist0 is not None:
        d = torch.zeros((G, 12), dtype=torch.float64, device=dev)
        d[:, :dist0.shape[1]] = dist0
        dist0 = d
    K, dist, R, t, rvec = f64(dev, G, 3, 3), f64(dev, G, 12), f64(dev, G, V, 3, 3), f64(dev, G, V, 3), f64(dev, G, V, 3)
    err, stats, rms, c0, c, std = f64(dev, G, V, n), f64(dev, G, V, 3), f64(dev, G), f64(dev, G), f64(dev, G), f64(dev, G, 12)
    ne, nv, nc, ok = i32(dev, G), i32(dev, G), i32(dev, G), i32(dev, G)
    nws = int(lib().skimi_calibrate_workspace_bytes(G, V, n))
    ws = workspace(dev, nws, at_least=8)
    check(lib().skimi_calibrate_camera(ptr(obj), ptr(img), ptr(use), ptr(K0), ptr(dist0), G, V, n, width, height, mask, int(max_evals),
                                       ptr(K), ptr(dist), ptr(R), ptr(t), ptr(rvec), ptr(err), ptr(stats), ptr(rms), ptr(c0), ptr(c),
                                       ptr(std), ptr(ne), ptr(nv), ptr(nc), ptr(ok), ptr(ws), nws, current_stream()),
          "skimi_calibrate_camera")
    return CalibrationResult(K, dist, R, t, rvec, err, stats[..., 0], stats[..., 1], stats[..., 2], rms, c0, c, std, ne, nv, nc,
                             ok.bool())
