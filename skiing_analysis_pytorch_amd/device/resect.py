"""Camera resection from 3D points and 2D keypoints, and the pose relative to a group's first view (csrc/resect.hip; C-ABI:
skimi_resect_workspace_bytes, skimi_resect_cameras, skimi_relative_pose): VideoPose3D/slove_rt_from_3d.py; rules:
DESIGN §2 "Resection".
"""
from __future__ import annotations

from typing import NamedTuple

import torch

from .._args import contig_as, f64, group_split, i32, on_device, shapes, to_dev, workspace
from .._lib import check, current_stream, lib, ptr

RESECT_LOSSES = {"linear": 0, "soft_l1": 1}


class ResectResult(NamedTuple):
    """resect_cameras' outputs (device tensors; G groups, V views, N points)."""
    R: torch.Tensor          # float64 [G, V, 3, 3]; NaN for a failed problem
    t: torch.Tensor          # float64 [G, V, 3]
    K: torch.Tensor          # float64 [G, V, 3, 3]: the K used (given, or inferred from the problem's keypoints)
    cost0: torch.Tensor      # float64 [G, V]: cost of the start
    cost: torch.Tensor       # float64 [G, V]
    n_evals: torch.Tensor    # int32 [G, V]: cost evaluations, the start's included
    n_points: torch.Tensor   # int32 [G, V]: the masked count
    success: torch.Tensor    # bool [G, V]: not failed and stopped by a criterion other than max_evals
    err: torch.Tensor        # float64 [V, N]: pixel error of the final pose, NaN for unused points
    mean_err: torch.Tensor   # float64 [G, V]
    rms_err: torch.Tensor    # float64 [G, V]
    max_err: torch.Tensor    # float64 [G, V]
    R_rel: torch.Tensor      # float64 [G, V, 3, 3] = R_v R_0^T
    t_rel: torch.Tensor      # float64 [G, V, 3] = t_v - R_rel t_0


def relative_pose(R: torch.Tensor, t: torch.Tensor):
    """R [G, V, 3, 3], t [G, V, 3] (float64, device) -> the pose of every view relative to view 0 of its group:
    R_rel = R_v R_0^T, t_rel = t_v - R_rel t_0 (slove_rt_from_3d.py:252-254), one small launch."""
    on_device("relative_pose", R, t)
    if R.dim() != 4 or tuple(R.shape[2:]) != (3, 3) or tuple(t.shape) != tuple(R.shape[:2]) + (3,):
        raise ValueError(f"relative_pose: need R [G, V, 3, 3] and t [G, V, 3], got {list(R.shape)}, {list(t.shape)}")
    R, t = contig_as(R, torch.float64), contig_as(t, torch.float64)
    R_rel, t_rel = torch.empty_like(R), torch.empty_like(t)
    check(lib().skimi_relative_pose(ptr(R), ptr(t), R.shape[0], R.shape[1], ptr(R_rel), ptr(t_rel), current_stream()),
          "skimi_relative_pose")
    return R_rel, t_rel


def group_problem(fn, X, x2d, K, conf, R0, t0, loss, group_size):
    """The prologue of resect_cameras and refine_cameras_points: X [N, 3], x2d [V, N, 2], the optional K [V, 3, 3], conf
    [V, N], R0 [G, V, 3, 3] and t0 [G, V, 3] (which go together) checked and made float64 -> (X, x2d, K, conf, R0, t0, N, V,
    group size, G)."""
    on_device(fn, X, x2d, K, conf, R0, t0)
    if loss not in RESECT_LOSSES:
        raise ValueError(f"{fn}: unknown loss {loss!r}; known: {list(RESECT_LOSSES)}")
    if X.dim() != 2 or X.shape[1] != 3 or x2d.dim() != 3 or x2d.shape[1:] != (X.shape[0], 2):
        raise ValueError(f"{fn}: need X [N, 3] and x2d [V, N, 2], got {list(X.shape)}, {list(x2d.shape)}")
    if (R0 is None) != (t0 is None):
        raise ValueError(f"{fn}: R0 and t0 go together")
    N, V = X.shape[0], x2d.shape[0]
    gs, G = group_split(N, group_size)
    shapes(fn, (("K", K, (V, 3, 3)), ("conf", conf, (V, N)), ("R0", R0, (G, V, 3, 3)), ("t0", t0, (G, V, 3))))
    return (*(to_dev(a, dev=X.device) for a in (X, x2d, K, conf, R0, t0)), N, V, gs, G)


def resect_cameras(X: torch.Tensor, x2d: torch.Tensor, K=None, conf=None, group_size=None, R0=None, t0=None,
                   loss: str = "linear", f_scale: float = 1.0, min_conf: float = 0.0, max_evals: int = 200) -> ResectResult:
    """Each camera's (R, t) from 3D points and their 2D keypoints, in one launch: X [N, 3], x2d [V, N, 2] pixels, K
    [V, 3, 3] or None (inferred from the keypoints' spread), conf [V, N] detector scores or None -> ResectResult.  The
    points are cut into N / group_size consecutive groups (default: one group) and every (group, view) pair is solved on
    its own: group_size = N gives one pose per clip, group_size = J one per step.  Per problem: the points finite in X and
    in every view's keypoint whose weights (scores clipped to [0, 1]) reach min_conf; a DLT resection as the start unless
    R0 [G, V, 3, 3], t0 [G, V, 3] are given; Levenberg-Marquardt on the weighted reprojection residuals with loss
    "linear" or "soft_l1" (scipy's, scale f_scale) until the step vanishes or max_evals cost evaluations are spent (the
    start and every trial count; the fresh linearisation after an accepted trial does not).
    Fewer than 6 usable points or a non-finite start: R, t NaN and success False.  Rules: DESIGN §2 "Resection"."""
    X, x2d, K, conf, R0, t0, N, V, gs, G = group_problem("resect_cameras", X, x2d, K, conf, R0, t0, loss, group_size)
    dev = X.device
    R, t, Ko, c0, c = f64(dev, G, V, 3, 3), f64(dev, G, V, 3), f64(dev, G, V, 3, 3), f64(dev, G, V), f64(dev, G, V)
    err, stats, ne, npts, ok = f64(dev, V, N), f64(dev, G, V, 3), i32(dev, G, V), i32(dev, G, V), i32(dev, G, V)
    nws = int(lib().skimi_resect_workspace_bytes(N, V, gs))
    ws = workspace(dev, nws, optional=True)
    check(lib().skimi_resect_cameras(ptr(X), ptr(x2d), ptr(conf), ptr(K), ptr(R0), ptr(t0), N, V, gs, RESECT_LOSSES[loss],
                                     float(f_scale), float(min_conf), int(max_evals), ptr(R), ptr(t), ptr(Ko), ptr(c0), ptr(c),
                                     ptr(ne), ptr(npts), ptr(ok), ptr(err), ptr(stats), ptr(ws), nws, current_stream()),
          "skimi_resect_cameras")
    R_rel, t_rel = relative_pose(R, t)
    return ResectResult(R, t, Ko, c0, c, ne, npts, ok.bool(), err, stats[..., 0], stats[..., 1], stats[..., 2], R_rel, t_rel)
