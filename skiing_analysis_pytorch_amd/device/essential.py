"""The essential matrix between two calibrated views and the pose from it (csrc/essential.hip; C-ABI:
skimi_essential_workspace_bytes, skimi_essential_ransac, skimi_five_point): VideoPose3D/slove_rt_from_3d.py --init
essential, camera_position.py; rules: DESIGN §2 "Essential matrix".
"""
from __future__ import annotations

from typing import NamedTuple

import torch

from .._args import f64, group_split, i32, on_device, shapes, to_dev, u8, workspace
from .._lib import check, current_stream, lib, ptr


class EssentialResult(NamedTuple):
    """essential_ransac's outputs (device tensors; G groups, N points)."""
    R: torch.Tensor            # float64 [G, 3, 3]: X1 = R X0 + t; NaN for a failed group
    t: torch.Tensor            # float64 [G, 3] = baseline t^, ||t^|| = 1
    E: torch.Tensor            # float64 [G, 3, 3] = [t^]x R: b^T E a = 0
    inliers: torch.Tensor      # uint8 [N]: the winner's inliers; 0 for unused points
    pose_mask: torch.Tensor    # uint8 [N]: the inliers in front of both cameras of the chosen pose
    n_used: torch.Tensor       # int32 [G]: the masked count m
    n_inliers: torch.Tensor    # int32 [G]
    n_pose: torch.Tensor       # int32 [G]
    cheirality: torch.Tensor   # int32 [G, 4]: the four candidates' votes
    cost: torch.Tensor         # float64 [G]: the winner's truncated Sampson cost, normalised units
    winner: torch.Tensor       # int32 [G, 2]: (hypothesis, solution); -1 for a failed group
    n_solutions: torch.Tensor  # int32 [G]: all kept candidates of the group
    confidence: torch.Tensor   # float64 [G] = 1 - (1 - w^5)^H, w = n_inliers / m
    success: torch.Tensor      # bool [G]


def essential_ransac(x2d: torch.Tensor, K: torch.Tensor, conf=None, min_conf: float = 0.0, group_size=None,
                     threshold: float = 1.0, hypotheses: int = 1024, seed: int = 0, group_offset: int = 0,
                     baseline: float = 1.0, distance_thresh: float = 50.0) -> EssentialResult:
    """The essential matrix between two calibrated views and the pose from it, for many problems in one call: x2d
    [2, N, 2] pixels, K [2, 3, 3] (each view normalised through its own), conf [2, N] detector scores or None ->
    EssentialResult.  The correspondences are cut into N / group_size consecutive groups (default: one).  Per group: the
    points finite in both views whose weights reach min_conf; `hypotheses` five-point samples from a counter-based stream
    (seed, group + group_offset, hypothesis), all solved and all scored against every used point by the Sampson error
    with `threshold` pixels (no early termination); the solution with the most inliers, then the smaller truncated cost,
    wins; its four pose candidates are voted on by the inliers' depths (both > 0 and < distance_thresh).  Fewer than 5
    used points or no solution: R, t, E NaN, success False.  There is no refit and no scale: ||t|| = baseline.
    Rules: DESIGN §2 "Essential matrix"."""
    on_device("essential_ransac", x2d, K, conf)
    if x2d.dim() != 3 or x2d.shape[0] != 2 or x2d.shape[2] != 2 or tuple(K.shape) != (2, 3, 3):
        raise ValueError(f"essential_ransac: need x2d [2, N, 2] and K [2, 3, 3], got {list(x2d.shape)}, {list(K.shape)}")
    N = x2d.shape[1]
    shapes("essential_ransac", (("conf", conf, (2, N)),))
    gs, G = group_split(N, group_size)
    dev = x2d.device
    x2d, K, conf = (to_dev(a, dev=dev) for a in (x2d, K, conf))
    R, t, E, cost, confd = f64(dev, G, 3, 3), f64(dev, G, 3), f64(dev, G, 3, 3), f64(dev, G), f64(dev, G)
    inl, pm = u8(dev, N), u8(dev, N)
    nu, ni, npose, ch, win, ns, ok = i32(dev, G), i32(dev, G), i32(dev, G), i32(dev, G, 4), i32(dev, G, 2), i32(dev, G), i32(dev, G)
    nws = int(lib().skimi_essential_workspace_bytes(N, gs, int(hypotheses)))
    ws = workspace(dev, nws, at_least=8)
    check(lib().skimi_essential_ransac(ptr(x2d), ptr(conf), ptr(K), N, gs, float(min_conf), float(threshold), int(hypotheses),
                                       int(seed) & 0xFFFFFFFFFFFFFFFF, int(group_offset), float(baseline), float(distance_thresh),
                                       ptr(R), ptr(t), ptr(E), ptr(inl), ptr(pm), ptr(nu), ptr(ni), ptr(npose), ptr(ch), ptr(cost),
                                       ptr(win), ptr(ns), ptr(confd), ptr(ok), ptr(ws), nws, current_stream()),
          "skimi_essential_ransac")
    return EssentialResult(R, t, E, inl, pm, nu, ni, npose, ch, cost, win, ns, confd, ok.bool())


def five_point(a: torch.Tensor, b: torch.Tensor):
    """The five-point solver alone, one thread per sample: a, b [S, 5, 2] normalised coordinates (float64, device) -> (E
    [S, 10, 3, 3] with b^T E a = 0, ||E||_F = sqrt 2, a sample's solutions by x ascending and NaN beyond its count,
    counts [S] int32).  DESIGN §2 "Essential matrix", rule 4."""
    on_device("five_point", a, b)
    if a.dim() != 3 or tuple(a.shape[1:]) != (5, 2) or a.shape != b.shape:
        raise ValueError(f"five_point: need a, b [S, 5, 2], got {list(a.shape)}, {list(b.shape)}")
    a, b = to_dev(a), to_dev(b)
    S = a.shape[0]
    E, counts = f64(a.device, S, 10, 3, 3), i32(a.device, S)
    check(lib().skimi_five_point(ptr(a), ptr(b), S, ptr(E), ptr(counts), current_stream()), "skimi_five_point")
    return E, counts
