"""The cameras of a group and its 3D points refined together (csrc/refine.hip; C-ABI: skimi_refine_workspace_bytes,
skimi_refine_cameras_points): VideoPose3D/slove_rt_from_3d.py --refine camera_points; rules: DESIGN §2 "Camera + points
refinement".
"""
from __future__ import annotations

from typing import NamedTuple

import torch

from .._args import f64, i32, workspace
from .._lib import check, current_stream, lib, ptr
from .resect import RESECT_LOSSES, group_problem, relative_pose, resect_cameras


class RefineResult(NamedTuple):
    """refine_cameras_points' outputs (device tensors; G groups, V views, N points)."""
    R: torch.Tensor          # float64 [G, V, 3, 3]; NaN for a failed group
    t: torch.Tensor          # float64 [G, V, 3]
    K: torch.Tensor          # float64 [G, V, 3, 3]: the K used (given, or inferred from the group's keypoints)
    X_opt: torch.Tensor      # float64 [N, 3]: the refined points; unused points and failed groups keep X bit for bit
    cost0: torch.Tensor      # float64 [G]: cost of the start
    cost: torch.Tensor       # float64 [G]
    n_evals: torch.Tensor    # int32 [G]: cost evaluations, the start's included
    n_points: torch.Tensor   # int32 [G]: the masked count
    success: torch.Tensor    # bool [G]: not failed and stopped by a criterion other than max_evals
    err: torch.Tensor        # float64 [V, N]: pixel error of the final cameras at X_opt, NaN for unused points
    mean_err: torch.Tensor   # float64 [G, V]
    rms_err: torch.Tensor    # float64 [G, V]
    max_err: torch.Tensor    # float64 [G, V]
    moved: torch.Tensor      # float64 [G]: rms ||X_opt - X|| over the used points
    R_rel: torch.Tensor      # float64 [G, V, 3, 3] = R_v R_0^T
    t_rel: torch.Tensor      # float64 [G, V, 3] = t_v - R_rel t_0


def refine_cameras_points(X: torch.Tensor, x2d: torch.Tensor, K=None, R0=None, t0=None, conf=None, group_size=None,
                          lambda_x: float = 0.0, loss: str = "linear", f_scale: float = 1.0, min_conf: float = 0.0,
                          max_evals: int = 200) -> RefineResult:
    """The cameras of a group and its 3D points refined together, in one launch: X [N, 3], x2d [V, N, 2] pixels (V <= 4), K
    [V, 3, 3] or None (inferred per group), R0 [G, V, 3, 3] and t0 [G, V, 3] or None (then the DLT start of
    resect_cameras(..., max_evals=1)), conf [V, N] or None -> RefineResult.  The points are cut into N / group_size
    consecutive groups (default: one); per group a Levenberg-Marquardt over all its cameras and used points on the weighted
    reprojection residuals plus, when lambda_x > 0, the prior sqrt(lambda_x) (X - X0), with loss "linear" or "soft_l1"
    (scipy's, per component, scale f_scale); the step is solved exactly through the Schur complement on the points.  With
    lambda_x = 0 the solution is determined up to a similarity only: costs, err and the statistics are then what is
    promised, not R, t, X_opt themselves.  Fewer than 6 usable points or a non-finite start: R, t NaN, success False, the
    group's X_opt = X.  Rules: DESIGN §2 "Camera + points refinement"."""
    X, x2d, K, conf, R0, t0, N, V, gs, G = group_problem("refine_cameras_points", X, x2d, K, conf, R0, t0, loss, group_size)
    dev = X.device
    if R0 is None and G >= 1 and 1 <= V <= 4:
        r0 = resect_cameras(X, x2d, K=K, conf=conf, group_size=gs, loss=loss, f_scale=f_scale, min_conf=min_conf, max_evals=1)
        R0, t0 = r0.R, r0.t            # NaN where the resection failed: the group then fails here too
    R, t, Ko, Xo, err, stats = f64(dev, G, V, 3, 3), f64(dev, G, V, 3), f64(dev, G, V, 3, 3), f64(dev, N, 3), f64(dev, V, N), f64(dev, G, V, 3)
    c0, c, moved, ne, npts, ok = f64(dev, G), f64(dev, G), f64(dev, G), i32(dev, G), i32(dev, G), i32(dev, G)
    nws = int(lib().skimi_refine_workspace_bytes(N, V, gs))
    ws = workspace(dev, nws, at_least=8)
    check(lib().skimi_refine_cameras_points(ptr(X), ptr(x2d), ptr(conf), ptr(K), ptr(R0), ptr(t0), N, V, gs, float(lambda_x),
                                            RESECT_LOSSES[loss], float(f_scale), float(min_conf), int(max_evals), ptr(R), ptr(t),
                                            ptr(Ko), ptr(Xo), ptr(c0), ptr(c), ptr(ne), ptr(npts), ptr(ok), ptr(err), ptr(stats),
                                            ptr(moved), ptr(ws), nws, current_stream()),
          "skimi_refine_cameras_points")
    R_rel, t_rel = relative_pose(R, t)
    return RefineResult(R, t, Ko, Xo, c0, c, ne, npts, ok.bool(), err, stats[..., 0], stats[..., 1], stats[..., 2], moved,
                        R_rel, t_rel)
