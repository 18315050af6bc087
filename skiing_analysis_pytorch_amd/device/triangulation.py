"""Cameras from the pose encoding, depth unprojection and the three triangulations (csrc/geometry.hip; C-ABI:
skimi_pose_to_cameras, skimi_unproject_depth, skimi_triangulate_dlt, skimi_triangulate_triage, skimi_triangulate_robust).

Reference: vggt/vggt/utils/pose_enc.py:62-124, rotation.py:14-44, geometry.py:15-117, vggt/triangulate.py:13-71,
vggt/reproject.py:108-144 + triangulation/postprocess.py:70-121 (triage).
"""
from __future__ import annotations

from typing import NamedTuple

import torch

from .._args import contig_as, f32, f64, on_device, shapes, u8
from .._lib import check, current_stream, lib, ptr
from .lens import _undistorted_f32


def pose_encoding_to_extri_intri(pose_encoding: torch.Tensor, image_size_hw, build_intrinsics=True):
    """[B, S, 9] -> (extrinsics [B, S, 3, 4], intrinsics [B, S, 3, 3] | None); device tensors."""
    on_device("pose_encoding_to_extri_intri", pose_encoding, what="a device tensor")
    pe = contig_as(pose_encoding)
    lead = pe.shape[:-1]
    rows = pe.numel() // 9
    H, W = image_size_hw
    E = f32(pe.device, *lead, 3, 4)
    K = f32(pe.device, *lead, 3, 3) if build_intrinsics else None
    check(lib().skimi_pose_to_cameras(ptr(pe), rows, int(H), int(W), ptr(E), ptr(K), current_stream()),
          "skimi_pose_to_cameras")
    return E, K


def unproject_depth_map_to_point_map(depth: torch.Tensor, extrinsic: torch.Tensor, intrinsic: torch.Tensor):
    """depth [S, H, W, 1] | [S, H, W], E [S, 3, 4], K [S, 3, 3] -> world points [S, H, W, 3] (device)."""
    if depth.dim() == 4:
        depth = depth[..., 0]
    d = contig_as(depth)
    S, H, W = d.shape
    out = f32(d.device, S, H, W, 3)
    E, K = contig_as(extrinsic), contig_as(intrinsic)
    check(lib().skimi_unproject_depth(ptr(d), ptr(E), ptr(K), ptr(out), S, H, W, current_stream()),
          "skimi_unproject_depth")
    return out


def triangulate_joints(K: torch.Tensor, R: torch.Tensor, t: torch.Tensor, keypoints: torch.Tensor):
    """K, R [T, V, 3, 3], t [T, V, 3], keypoints [T, V, J, 2] (pixels) -> [T, J, 3].
    V = 2 is the reference's triangulate_one_frame; V > 2 stacks two DLT rows per view."""
    on_device("triangulate_joints", K, R, t, keypoints)
    T, V, J, _ = keypoints.shape
    K, R, t, kp = (contig_as(a) for a in (K, R, t, keypoints))
    out = f32(kp.device, T, J, 3)
    check(lib().skimi_triangulate_dlt(ptr(K), ptr(R), ptr(t), ptr(kp), ptr(out), T, V, J, current_stream()),
          "skimi_triangulate_dlt")
    return out


class TriageResult(NamedTuple):
    """triangulate_triage's outputs (device tensors; T steps, V views, J joints)."""
    X: torch.Tensor            # float32 [T, J, 3]: triangulate_joints' result
    X_clean: torch.Tensor      # float32 [T, J, 3]: X where kept, NaN elsewhere
    err: torch.Tensor          # float64 [T, V, J]: reprojection error in pixels
    depth: torch.Tensor        # float64 [T, V, J]: depth of X in each view's camera
    keep: torch.Tensor         # bool [T, J]
    view_stats: torch.Tensor   # float64 [T, V, 4]: VIEW_STAT_FIELDS of err over the joints (NaN-aware)
    report: torch.Tensor       # float64 [T, 5]: rmse_px, median_err_px, pos_depth_ratio, kept_ratio, kept_count (postprocess.py:115-121)


VIEW_STAT_FIELDS = ("rmse", "mean_err", "median_err", "max_err")   # vggt/reproject.py:334-341


def _steps(fn, kp):
    if kp.dim() != 4 or kp.shape[-1] != 2:
        raise ValueError(f"{fn}: keypoints must be [T, V, J, 2], got {list(kp.shape)}")
    return kp.shape[:3]


def _prepared_rows(K, R, t, kp, conf, T, V, J):
    """the shape table of the two launches: their tensors come prepared and are not converted"""
    return (("K", K, (T, V, 3, 3)), ("R", R, (T, V, 3, 3)), ("t", t, (T, V, 3)), ("keypoints", kp, (T, V, J, 2)),
            ("conf", conf, (T, V, J)))


def _prepare(fn, K, R, t, keypoints, conf, dist):
    """what triangulate_triage and triangulate_robust hand to their launch: float32, contiguous, keypoints undistorted"""
    on_device(fn, K, R, t, keypoints, conf)
    K, R, t, kp, conf = (contig_as(a) for a in (K, R, t, keypoints, conf))
    return K, R, t, _undistorted_f32(kp, K, dist), conf


def triage_launch(K, R, t, kp, conf, conf_thr, err_thresh_px):
    """the launch of triangulate_triage on prepared float32 device tensors; keep stays uint8 (it travels in the packed
    all-gather of infer.process_multi_view_clip that way)"""
    T, V, J = _steps("triangulate_triage", kp)
    dev = kp.device
    shapes("triangulate_triage", _prepared_rows(K, R, t, kp, conf, T, V, J), f32_on=dev)
    X, Xc, err, depth = f32(dev, T, J, 3), f32(dev, T, J, 3), f64(dev, T, V, J), f64(dev, T, V, J)
    keep, vs, rep = u8(dev, T, J), f64(dev, T, V, 4), f64(dev, T, 5)
    check(lib().skimi_triangulate_triage(ptr(K), ptr(R), ptr(t), ptr(kp), ptr(conf), float(conf_thr), float(err_thresh_px),
                                         T, V, J, ptr(X), ptr(Xc), ptr(err), ptr(depth), ptr(keep), ptr(vs), ptr(rep),
                                         current_stream()), "skimi_triangulate_triage")
    return X, Xc, err, depth, keep, vs, rep


def triangulate_triage(K: torch.Tensor, R: torch.Tensor, t: torch.Tensor, keypoints: torch.Tensor, conf=None,
                       conf_thr: float = 0.3, err_thresh_px: float = 2.0, dist=None) -> TriageResult:
    """triangulate_joints with a verdict, in one launch: K, R [T, V, 3, 3], t [T, V, 3], keypoints [T, V, J, 2] (pixels),
    conf [T, V, J] detector scores or None -> TriageResult (unpacks as X, X_clean, err, depth, keep, view_stats, report).
    Every view is projected through its own (K, R, t): err = ||K (R X + t) / depth - keypoint||, em = mean over the views;
    a joint is kept iff every depth > 0, em is finite and <= err_thresh_px, and every score >= conf_thr
    (post_triage_single, triangulation/postprocess.py:70-121, from two views to V).  2 <= V <= 8, 1 <= J <= 32.
    dist: None, or the lens coefficients of the views ([k] or [V, k], host; lens_coeffs): the keypoints are first undistorted
    with their view's K, undistortPoints(x, K, d, P=K) as post_triage_single's dist1 / dist2 (one more launch in front;
    the triage kernel is the same).  None or all-zero coefficients: exactly the call without dist."""
    K, R, t, kp, conf = _prepare("triangulate_triage", K, R, t, keypoints, conf, dist)
    X, Xc, err, depth, keep, vs, rep = triage_launch(K, R, t, kp, conf, conf_thr, err_thresh_px)
    return TriageResult(X, Xc, err, depth, keep.bool(), vs, rep)


class RobustResult(NamedTuple):
    """triangulate_robust's outputs (device tensors; T steps, V views, J joints), in the order of rule 7."""
    joints3d: torch.Tensor           # float32 [T, J, 3]: the consensus X; NaN x 3 for a failed joint
    err: torch.Tensor                # float64 [T, V, J]: reprojection error of X in every view with finite keypoints
    inlier_views: torch.Tensor       # uint8 [T, J]: bit v = view v is in the final inlier set (0: failed)
    rms_px: torch.Tensor             # float64 [T, J]: sqrt(mean over the set of err^2)
    ok: torch.Tensor                 # bool [T, J]: not failed, popcount(inlier_views) >= min_inliers, X finite
    joints3d_ok: torch.Tensor        # float32 [T, J, 3]: joints3d where ok, NaN elsewhere (what fuse.smooth_skeleton takes)
    view_inlier_ratio: torch.Tensor  # float64 [T, V]: share of the joints that did not fail which hold view v
    report: torch.Tensor             # float64 [T, 4]: ok count, ok ratio, mean popcount and rms of rms_px over the ok joints


ROBUST_MAX_VIEWS, ROBUST_MAX_JOINTS, ROBUST_MAX_REFINE_ITERS = 8, 32, 32


def robust_launch(K, R, t, kp, conf, conf_thr, inlier_px, min_inliers, refine_iters, weighted):
    """the launch of triangulate_robust on prepared float32 device tensors; ok stays uint8 (it travels in the packed
    all-gather of infer.process_multi_view_clip that way).  Everything is checked before the launch."""
    T, V, J = _steps("triangulate_robust", kp)
    if T < 1 or not 2 <= V <= ROBUST_MAX_VIEWS or not 1 <= J <= ROBUST_MAX_JOINTS:
        raise ValueError(f"triangulate_robust: need T >= 1, 2..{ROBUST_MAX_VIEWS} views and 1..{ROBUST_MAX_JOINTS} joints, "
                         f"got keypoints {list(kp.shape)}")
    min_inliers, refine_iters = int(min_inliers), int(refine_iters)
    if not 2 <= min_inliers <= V:
        raise ValueError(f"triangulate_robust: min_inliers must be in 2..{V} (the views), got {min_inliers}")
    if not 0 <= refine_iters <= ROBUST_MAX_REFINE_ITERS:
        raise ValueError(f"triangulate_robust: refine_iters must be in 0..{ROBUST_MAX_REFINE_ITERS}, got {refine_iters}")
    if not float(inlier_px) >= 0:
        raise ValueError(f"triangulate_robust: inlier_px must be >= 0, got {inlier_px}")
    dev = kp.device
    shapes("triangulate_robust", _prepared_rows(K, R, t, kp, conf, T, V, J), f32_on=dev)
    X, err, inl, rms = f32(dev, T, J, 3), f64(dev, T, V, J), u8(dev, T, J), f64(dev, T, J)
    ok, Xok, ratio, rep = u8(dev, T, J), f32(dev, T, J, 3), f64(dev, T, V), f64(dev, T, 4)
    check(lib().skimi_triangulate_robust(ptr(K), ptr(R), ptr(t), ptr(kp), ptr(conf), float(conf_thr), float(inlier_px),
                                         min_inliers, refine_iters, 1 if weighted else 0, T, V, J, ptr(X), ptr(err), ptr(inl),
                                         ptr(rms), ptr(ok), ptr(Xok), ptr(ratio), ptr(rep), current_stream()),
          "skimi_triangulate_robust")
    return X, err, inl, rms, ok, Xok, ratio, rep


def triangulate_robust(K: torch.Tensor, R: torch.Tensor, t: torch.Tensor, keypoints: torch.Tensor, conf=None,
                       conf_thr: float = 0.3, inlier_px: float = 2.0, min_inliers: int = 2, refine_iters: int = 5,
                       weighted: bool = False, dist=None) -> RobustResult:
    """Outlier-robust triangulation in one launch: K, R [T, V, 3, 3], t [T, V, 3], keypoints [T, V, J, 2] (pixels), conf
    [T, V, J] detector scores or None -> RobustResult.  Per joint: every pair of eligible views (finite keypoint, score >=
    conf_thr) gives a two-view DLT hypothesis; the one with the most views within inlier_px (then the smaller truncated
    cost, then the earlier pair) wins; up to three DLT refits over its inlier set, then refine_iters Gauss-Newton steps on
    the reprojection error of that set.  weighted=True weights refit and refinement by the scores clipped to [0, 1].  A
    joint with fewer than two agreeing views fails (NaN); `ok` also asks for min_inliers views in the final set.  With
    every view an inlier, refine_iters=0 and no weighting the result is triangulate_joints'.  Rules: DESIGN §2 "Robust
    triangulation".  2 <= V <= 8, 1 <= J <= 32, 2 <= min_inliers <= V, 0 <= refine_iters <= 32.  dist: None, or the views'
    lens coefficients ([k] or [V, k], host): the keypoints are first undistorted with their view's K, as in
    triangulate_triage; None or all-zero coefficients: exactly the call without dist."""
    K, R, t, kp, conf = _prepare("triangulate_robust", K, R, t, keypoints, conf, dist)
    X, err, inl, rms, ok, Xok, ratio, rep = robust_launch(K, R, t, kp, conf, conf_thr, inlier_px, min_inliers, refine_iters,
                                                          weighted)
    return RobustResult(X, err, inl, rms, ok.bool(), Xok, ratio, rep)
