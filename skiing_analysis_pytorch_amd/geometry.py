"""Device-side geometry post-processing (C-ABI: skimi_pose_to_cameras, skimi_unproject_depth,
skimi_triangulate_dlt, skimi_triangulate_triage, skimi_triangulate_robust, the person origin: skimi_person_origin, skimi_recenter_cameras,
and the point-to-plane ICP: skimi_estimate_normals, skimi_icp_correspondences,
skimi_icp_point_to_plane; the bundle adjustment: skimi_bundle_adjust; the camera resection: skimi_resect_cameras, the camera-and-points refinement: skimi_refine_cameras_points,
skimi_relative_pose; the essential matrix: skimi_essential_ransac, skimi_five_point; the fusion and smoothing of a clip:
skimi_fuse_h36m, skimi_fuse_views, skimi_smooth_ema, skimi_smooth_savgol; the kinematic analysis of clips: skimi_kinematics;
the lens model on points: skimi_distort_points, skimi_undistort_points, skimi_project_points; the bird's-eye view:
skimi_homography_fit, skimi_homography_points, skimi_bev_skeleton, skimi_ground_track; the camera calibration:
skimi_calibrate_camera)
plus the small host helpers of the reference's VGGT wrapper.

Reference: vggt/vggt/utils/pose_enc.py:62-124, rotation.py:14-44, geometry.py:15-117,
vggt/triangulate.py:13-71, vggt/reproject.py:108-144 + triangulation/postprocess.py:70-121 (triage),
vggt/multi_view_process.py:195-217 + :356-395 (person origin), vggt/vggt/infer.py:107-155, vggt/multi_view_process.py:427-520 (ICP),
:523-564 + bundle_adjustment/loss.py (bundle adjustment), VideoPose3D/slove_rt_from_3d.py (resection),
VideoPose3D/fuse/fuse.py, fuse/main_raw.py:194-250, fuse/fuse.py:289-412 (fusion and smoothing; host form: fuse.py),
angle/main.py (kinematics; entry points: angle.py), camera_calibration/calibration_parameters.* + triangulation/postprocess.py:89-97
(lens distortion, from OpenCV's documented model), front_side/front/bev_utils.py + front_side/run.py:153-197, :222-255
(bird's-eye view; the reference's names: bev.py), camera_calibration/main.py (calibration; the reference's names: calibration.py).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from ._lib import check, lib, ptr


def pose_encoding_to_extri_intri(pose_encoding: torch.Tensor, image_size_hw, build_intrinsics=True):
    """[B, S, 9] -> (extrinsics [B, S, 3, 4], intrinsics [B, S, 3, 3] | None); device tensors."""
    if not pose_encoding.is_cuda:
        raise _lib.SkimiError("pose_encoding_to_extri_intri needs a device tensor")
    pe = pose_encoding.contiguous().to(torch.float32)
    lead = pe.shape[:-1]
    rows = pe.numel() // 9
    H, W = image_size_hw
    E = torch.empty((*lead, 3, 4), dtype=torch.float32, device=pe.device)
    K = torch.empty((*lead, 3, 3), dtype=torch.float32, device=pe.device) if build_intrinsics else None
    check(lib().skimi_pose_to_cameras(ptr(pe), rows, int(H), int(W), ptr(E), ptr(K), _lib.current_stream()),
          "skimi_pose_to_cameras")
    return E, K


def unproject_depth_map_to_point_map(depth: torch.Tensor, extrinsic: torch.Tensor, intrinsic: torch.Tensor):
    """depth [S, H, W, 1] | [S, H, W], E [S, 3, 4], K [S, 3, 3] -> world points [S, H, W, 3] (device)."""
    if depth.dim() == 4:
        depth = depth[..., 0]
    d = depth.contiguous().to(torch.float32)
    S, H, W = d.shape
    out = torch.empty((S, H, W, 3), dtype=torch.float32, device=d.device)
    E = extrinsic.contiguous().to(torch.float32)
    K = intrinsic.contiguous().to(torch.float32)
    check(lib().skimi_unproject_depth(ptr(d), ptr(E), ptr(K), ptr(out), S, H, W, _lib.current_stream()),
          "skimi_unproject_depth")
    return out


def triangulate_joints(K: torch.Tensor, R: torch.Tensor, t: torch.Tensor, keypoints: torch.Tensor):
    """K, R [T, V, 3, 3], t [T, V, 3], keypoints [T, V, J, 2] (pixels) -> [T, J, 3].
    V = 2 is the reference's triangulate_one_frame; V > 2 stacks two DLT rows per view."""
    for a in (K, R, t, keypoints):
        if not a.is_cuda:
            raise _lib.SkimiError("triangulate_joints needs device tensors")
    T, V, J, _ = keypoints.shape
    K, R, t = (a.contiguous().to(torch.float32) for a in (K, R, t))
    kp = keypoints.contiguous().to(torch.float32)
    out = torch.empty((T, J, 3), dtype=torch.float32, device=kp.device)
    check(lib().skimi_triangulate_dlt(ptr(K), ptr(R), ptr(t), ptr(kp), ptr(out), T, V, J, _lib.current_stream()),
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


def triage_launch(K, R, t, kp, conf, conf_thr, err_thresh_px):
    """the launch of triangulate_triage on prepared float32 device tensors; keep stays uint8 (it travels in the packed
    all-gather of infer.process_multi_view_clip that way)"""
    if kp.dim() != 4 or kp.shape[-1] != 2:
        raise ValueError(f"triangulate_triage: keypoints must be [T, V, J, 2], got {list(kp.shape)}")
    T, V, J, _ = kp.shape
    dev = kp.device
    want = {"K": (T, V, 3, 3), "R": (T, V, 3, 3), "t": (T, V, 3), "keypoints": (T, V, J, 2), "conf": (T, V, J)}
    for name, a in (("K", K), ("R", R), ("t", t), ("keypoints", kp), ("conf", conf)):
        if a is None:
            continue
        if not a.is_cuda or a.device != dev:
            raise _lib.SkimiError(f"triangulate_triage needs device tensors on one device ({name} is on {a.device})")
        if tuple(a.shape) != want[name] or a.dtype != torch.float32 or not a.is_contiguous():
            raise ValueError(f"triangulate_triage: {name} must be contiguous float32 {list(want[name])}, got {a.dtype} "
                             f"{list(a.shape)}")
    X = torch.empty((T, J, 3), dtype=torch.float32, device=dev)
    Xc = torch.empty((T, J, 3), dtype=torch.float32, device=dev)
    err = torch.empty((T, V, J), dtype=torch.float64, device=dev)
    depth = torch.empty((T, V, J), dtype=torch.float64, device=dev)
    keep = torch.empty((T, J), dtype=torch.uint8, device=dev)
    vs = torch.empty((T, V, 4), dtype=torch.float64, device=dev)
    rep = torch.empty((T, 5), dtype=torch.float64, device=dev)
    check(lib().skimi_triangulate_triage(ptr(K), ptr(R), ptr(t), ptr(kp), ptr(conf), float(conf_thr), float(err_thresh_px),
                                         T, V, J, ptr(X), ptr(Xc), ptr(err), ptr(depth), ptr(keep), ptr(vs), ptr(rep),
                                         _lib.current_stream()), "skimi_triangulate_triage")
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
    for a in (K, R, t, keypoints) + (() if conf is None else (conf,)):
        if not a.is_cuda:
            raise _lib.SkimiError("triangulate_triage needs device tensors")
    K, R, t = (a.contiguous().to(torch.float32) for a in (K, R, t))
    kp = keypoints.contiguous().to(torch.float32)
    if conf is not None:
        conf = conf.contiguous().to(torch.float32)
    kp = _undistorted_f32(kp, K, dist)
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
    if kp.dim() != 4 or kp.shape[-1] != 2:
        raise ValueError(f"triangulate_robust: keypoints must be [T, V, J, 2], got {list(kp.shape)}")
    T, V, J, _ = kp.shape
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
    want = {"K": (T, V, 3, 3), "R": (T, V, 3, 3), "t": (T, V, 3), "keypoints": (T, V, J, 2), "conf": (T, V, J)}
    for name, a in (("K", K), ("R", R), ("t", t), ("keypoints", kp), ("conf", conf)):
        if a is None:
            continue
        if not a.is_cuda or a.device != dev:
            raise _lib.SkimiError(f"triangulate_robust needs device tensors on one device ({name} is on {a.device})")
        if tuple(a.shape) != want[name] or a.dtype != torch.float32 or not a.is_contiguous():
            raise ValueError(f"triangulate_robust: {name} must be contiguous float32 {list(want[name])}, got {a.dtype} "
                             f"{list(a.shape)}")
    X = torch.empty((T, J, 3), dtype=torch.float32, device=dev)
    err = torch.empty((T, V, J), dtype=torch.float64, device=dev)
    inl = torch.empty((T, J), dtype=torch.uint8, device=dev)
    rms = torch.empty((T, J), dtype=torch.float64, device=dev)
    ok = torch.empty((T, J), dtype=torch.uint8, device=dev)
    Xok = torch.empty((T, J, 3), dtype=torch.float32, device=dev)
    ratio = torch.empty((T, V), dtype=torch.float64, device=dev)
    rep = torch.empty((T, 4), dtype=torch.float64, device=dev)
    check(lib().skimi_triangulate_robust(ptr(K), ptr(R), ptr(t), ptr(kp), ptr(conf), float(conf_thr), float(inlier_px),
                                         min_inliers, refine_iters, 1 if weighted else 0, T, V, J, ptr(X), ptr(err), ptr(inl),
                                         ptr(rms), ptr(ok), ptr(Xok), ptr(ratio), ptr(rep), _lib.current_stream()),
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
    for a in (K, R, t, keypoints) + (() if conf is None else (conf,)):
        if not a.is_cuda:
            raise _lib.SkimiError("triangulate_robust needs device tensors")
    K, R, t = (a.contiguous().to(torch.float32) for a in (K, R, t))
    kp = keypoints.contiguous().to(torch.float32)
    if conf is not None:
        conf = conf.contiguous().to(torch.float32)
    kp = _undistorted_f32(kp, K, dist)
    X, err, inl, rms, ok, Xok, ratio, rep = robust_launch(K, R, t, kp, conf, conf_thr, inlier_px, min_inliers, refine_iters,
                                                          weighted)
    return RobustResult(X, err, inl, rms, ok.bool(), Xok, ratio, rep)


@dataclass
class PersonOrigin:
    """person_origin's outputs (device tensors, one entry per map; lead = the maps' leading shape)."""
    origin: torch.Tensor    # float64 [..., 3]: mean of the kept points; NaN where nothing was kept
    n_valid: torch.Tensor   # int64 [...]: finite points inside the box
    n_kept: torch.Tensor    # int64 [...]: of those, within 3 sigma of the median depth
    median: torch.Tensor    # float64 [...]
    std: torch.Tensor       # float64 [...]
    stats: torch.Tensor     # float64 [..., 8]: the kernel's record (n_box, n_valid, n_kept, median, std, origin)


def person_stats(points: torch.Tensor, boxes: torch.Tensor, source_size) -> torch.Tensor:
    """the launch of person_origin: points [M, H, W, 3], boxes [M, 4], float32, contiguous, device -> stats [M, 8]"""
    M, H, W, _ = points.shape
    stats = torch.empty((M, 8), dtype=torch.float64, device=points.device)
    nws = int(lib().skimi_person_workspace_bytes(M, H, W))
    ws = torch.empty(nws, dtype=torch.uint8, device=points.device) if nws else None
    check(lib().skimi_person_origin(ptr(points), ptr(boxes), M, H, W, int(source_size[0]), int(source_size[1]), ptr(ws),
                                    ptr(stats), _lib.current_stream()), "skimi_person_origin")
    return stats


def person_origin(point_maps: torch.Tensor, boxes: torch.Tensor, source_size) -> PersonOrigin:
    """The person-centred origin of dense world-point maps (extract_person_points + the mean its caller takes,
    vggt/multi_view_process.py:356-395, :195-199) without leaving the device: point_maps [..., H, W, 3], boxes [..., 4]
    = (x1, y1, x2, y2) in the pixels of the `source_size` = (height, width) image the detector saw.  Per map: the
    pixels inside the scaled box, finite, within 3 sigma of their median depth (exact median, float64 statistics;
    DESIGN §2 "Person origin") -> their float64 mean."""
    if not point_maps.is_cuda or not boxes.is_cuda:
        raise _lib.SkimiError("person_origin needs device tensors")
    if point_maps.dim() < 3 or point_maps.shape[-1] != 3:
        raise _lib.SkimiError(f"person_origin: point_maps must be [..., H, W, 3], got {tuple(point_maps.shape)}")
    lead = tuple(point_maps.shape[:-3])
    if tuple(boxes.shape) != lead + (4,):
        raise _lib.SkimiError(f"person_origin: boxes must be {list(lead + (4,))}, got {list(boxes.shape)}")
    H, W = point_maps.shape[-3:-1]
    p = point_maps.reshape(-1, H, W, 3).contiguous().to(torch.float32)
    b = boxes.reshape(-1, 4).contiguous().to(torch.float32)
    stats = person_stats(p, b, source_size).reshape(*lead, 8)
    return PersonOrigin(stats[..., 5:8], stats[..., 1].to(torch.int64), stats[..., 2].to(torch.int64), stats[..., 3],
                        stats[..., 4], stats)


def recenter_cameras(stats: torch.Tensor, extrinsic: torch.Tensor):
    """The camera update that follows the person origins (multi_view_process.py:201-217), one small launch: stats
    [n, S, 8] (PersonOrigin.stats), extrinsic [n, S, 3, 4] float32 -> (origin [n, 3] float64 = mean of the S origins in
    view order, zero if a view kept nothing; R [n, S, 3, 3], t [n, S, 3] float32 with t_c += R_c origin and, at S = 2,
    view 1 turned by diag(-1, 1, -1) with its t left as the reference's turn-then-mirror leaves it)."""
    if not stats.is_cuda or not extrinsic.is_cuda:
        raise _lib.SkimiError("recenter_cameras needs device tensors")
    n, S = extrinsic.shape[:2]
    if tuple(stats.shape) != (n, S, 8) or tuple(extrinsic.shape[2:]) != (3, 4):
        raise ValueError(f"recenter_cameras: need stats [n, S, 8] and extrinsic [n, S, 3, 4], got {list(stats.shape)}, "
                         f"{list(extrinsic.shape)}")
    stats = stats.contiguous().to(torch.float64)
    E = extrinsic.contiguous().to(torch.float32)
    origin = torch.empty((n, 3), dtype=torch.float64, device=E.device)
    R = torch.empty((n, S, 3, 3), dtype=torch.float32, device=E.device)
    t = torch.empty((n, S, 3), dtype=torch.float32, device=E.device)
    check(lib().skimi_recenter_cameras(ptr(stats), ptr(E), n, S, ptr(origin), ptr(R), ptr(t), _lib.current_stream()),
          "skimi_recenter_cameras")
    return origin, R, t


# ---- the filtered, coloured scene cloud of a time step (predictions_to_glb restated; DESIGN §2 "Scene cloud") ----
SCENE_MAX_PIXELS = (2 ** 31 - 1) // 3


class SceneCloud(NamedTuple):
    """scene_point_cloud's outputs (device tensors, B scenes of n pixels, cap rows each)."""
    xyz: torch.Tensor          # float32 [B, cap, 3]: the kept vertices in pixel order (aligned or raw); rows >= count unwritten
    rgb: torch.Tensor          # uint8 [B, cap, 3]
    count: torch.Tensor        # int64 [B]: the full number kept (may exceed cap)
    threshold: torch.Tensor    # float64 [B]
    lower: torch.Tensor        # float64 [B, 3]: 5th percentile of the raw kept vertices per axis
    upper: torch.Tensor        # float64 [B, 3]: 95th
    scale: torch.Tensor        # float64 [B]: ||upper - lower||; 1 for an empty scene
    transform: torch.Tensor    # float64 [B, 4, 4]: E0^-1 diag(-1, -1, 1, 1)
    n_nan_conf: torch.Tensor   # int64 [B]
    n_nonfinite: torch.Tensor  # int64 [B]: kept vertices with a non-finite coordinate
    stats: torch.Tensor        # float64 [B, 16]: the kernel's record (thr, lo, hi, ...; include/skimi.h)


def scene_launch(n: int):
    """The launch geometry of scene_point_cloud for a scene of n pixels: (workgroups per scene, consecutive pixels each
    handles per pass)."""
    n = int(n)
    tile = int(lib().skimi_scene_tile(n))
    if tile <= 0:
        raise ValueError(f"scene_launch: a scene holds 1..{SCENE_MAX_PIXELS} pixels, got {n}")
    return (n + tile - 1) // tile, tile


def scene_point_cloud(points: torch.Tensor, conf: torch.Tensor, images: torch.Tensor, extrinsic: torch.Tensor,
                      conf_thres: float = 50.0, mask_black_bg: bool = False, mask_white_bg: bool = False, align: bool = True,
                      capacity=None, out=None) -> SceneCloud:
    """The point cloud predictions_to_glb builds (vggt/visual_util.py:39-236) for B time steps in one call, without
    leaving the device: points [B, S, H, W, 3], conf [B, S, H, W], images [B, S, 3, H, W] or [B, S, H, W, 3] (the
    reference's test: shape[2] == 3 means channels first), extrinsic [B, S, 3, 4].  Per scene: uint8 colours, the
    conf_thres-th percentile of the confidences as threshold (exact, float64), the kept pixels compacted in pixel order,
    the 5th / 95th percentile box of the kept vertices and its diagonal (the scene scale), and the alignment E0^-1
    diag(-1, -1, 1, 1), applied to the written vertices when align.  capacity (default S H W) bounds the rows written per
    scene; `count` is the full number kept.  out=(xyz, rgb): write into these tensors ([B, capacity, 3] float32 / uint8)
    instead of allocating them.  Rules: DESIGN §2 "Scene cloud"."""
    for name, a in (("points", points), ("conf", conf), ("images", images), ("extrinsic", extrinsic)):
        if not a.is_cuda:
            raise _lib.SkimiError(f"scene_point_cloud needs device tensors ({name} is on {a.device})")
    if points.dim() != 5 or points.shape[-1] != 3:
        raise ValueError(f"scene_point_cloud: points must be [B, S, H, W, 3], got {list(points.shape)}")
    B, S, H, W, _ = points.shape
    if B < 1 or S < 1 or H < 1 or W < 1:
        raise ValueError(f"scene_point_cloud: need B >= 1, S >= 1 and a non-empty map, got points {list(points.shape)}")
    n = S * H * W
    if n > SCENE_MAX_PIXELS:
        raise ValueError(f"scene_point_cloud: a scene holds at most {SCENE_MAX_PIXELS} pixels, got {n}")
    if tuple(conf.shape) != (B, S, H, W):
        raise ValueError(f"scene_point_cloud: conf must be {[B, S, H, W]}, got {list(conf.shape)}")
    if images.dim() != 5:
        raise ValueError(f"scene_point_cloud: images must be [B, S, 3, H, W] or [B, S, H, W, 3], got {list(images.shape)}")
    nchw = images.shape[2] == 3   # the reference's `images.shape[1] == 3` on one scene
    if tuple(images.shape) != ((B, S, 3, H, W) if nchw else (B, S, H, W, 3)):
        raise ValueError(f"scene_point_cloud: images must be [B, S, 3, H, W] or [B, S, H, W, 3] for points "
                         f"{list(points.shape)}, got {list(images.shape)}")
    if tuple(extrinsic.shape) != (B, S, 3, 4):
        raise ValueError(f"scene_point_cloud: extrinsic must be {[B, S, 3, 4]}, got {list(extrinsic.shape)}")
    q = float(conf_thres)
    if not 0.0 <= q <= 100.0:
        raise ValueError(f"scene_point_cloud: conf_thres is a percentile in [0, 100], got {conf_thres}")
    cap = n if capacity is None else int(capacity)
    if cap < 1:
        raise ValueError(f"scene_point_cloud: capacity must be at least 1, got {capacity}")
    dev = points.device
    points, conf, images, extrinsic = (a.contiguous().to(torch.float32) for a in (points, conf, images, extrinsic))
    if out is None:
        xyz = torch.empty((B, cap, 3), dtype=torch.float32, device=dev)
        rgb = torch.empty((B, cap, 3), dtype=torch.uint8, device=dev)
    else:
        xyz, rgb = out
        for a, dt in ((xyz, torch.float32), (rgb, torch.uint8)):
            if not a.is_cuda or a.dtype != dt or tuple(a.shape) != (B, cap, 3) or not a.is_contiguous():
                raise ValueError(f"scene_point_cloud: out must be contiguous device tensors {[B, cap, 3]} float32 / uint8")
    count = torch.empty((B,), dtype=torch.int64, device=dev)
    stats = torch.empty((B, 16), dtype=torch.float64, device=dev)
    transform = torch.empty((B, 4, 4), dtype=torch.float64, device=dev)
    ws = torch.empty(int(lib().skimi_scene_workspace_bytes(B, n)), dtype=torch.uint8, device=dev)
    check(lib().skimi_scene_cloud(ptr(points), ptr(conf), ptr(images), ptr(extrinsic), B, S, H, W, 1 if nchw else 0, q,
                                  1 if mask_black_bg else 0, 1 if mask_white_bg else 0, 1 if align else 0, cap, ptr(ws), ptr(xyz),
                                  ptr(rgb), ptr(count), ptr(stats), ptr(transform), _lib.current_stream()), "skimi_scene_cloud")
    return SceneCloud(xyz, rgb, count, stats[:, 0], stats[:, 5:8], stats[:, 8:11], stats[:, 11], transform,
                      stats[:, 3].to(torch.int64), stats[:, 4].to(torch.int64), stats)


# ---- point-to-plane ICP (Open3D's estimate_normals + registration_icp, restated; DESIGN §2 "ICP") ------------
# Rules where Open3D's result depends on its implementation: a point is valid iff its coordinates are finite and
# x^2 + y^2 + z^2 > 1e-12 (the reference keeps ||p|| > 1e-6, which lets inf points in: the two differ only on
# non-finite input); neighbours / correspondences lie at d^2 < r^2 in float64; a tie between equidistant target points
# goes to the smaller index; every sum has a fixed order (bitwise reproducible); normals are float64 eigenvectors
# solved to convergence (Jacobi), their sign arbitrary.
def _cloud(points: torch.Tensor, what: str) -> torch.Tensor:
    if not points.is_cuda:
        raise _lib.SkimiError(f"{what} needs a device tensor")
    if points.shape[-1] != 3:
        raise _lib.SkimiError(f"{what}: points must be [..., 3], got {tuple(points.shape)}")
    return points.reshape(-1, 3).contiguous().to(torch.float32)


def _icp_workspace(n_src: int, n_tgt: int, device) -> torch.Tensor:
    return torch.empty(int(lib().skimi_icp_workspace_bytes(n_src, n_tgt)), dtype=torch.uint8, device=device)


def _mat4(T) -> "C.Array":
    a = np.ascontiguousarray(np.asarray(T, dtype=np.float64).reshape(4, 4))
    return (C.c_double * 16)(*a.ravel().tolist())


def estimate_normals(points: torch.Tensor, radius: float = 0.05):
    """Radius normals (estimate_normals(KDTreeSearchParamRadius(radius)), multi_view_process.py:487-496) of a device
    cloud [..., 3] -> (normals float64 [N, 3], neighbour counts int32 [N]).  Neighbours are the valid points at
    d < radius, the point itself included; with >= 3 of them the normal is the smallest-eigenvalue eigenvector of their
    covariance, else (0, 0, 1).  Invalid points get (0, 0, 0) and 0."""
    p = _cloud(points, "estimate_normals")
    n = p.shape[0]
    normals = torch.empty((n, 3), dtype=torch.float64, device=p.device)
    counts = torch.empty((n,), dtype=torch.int32, device=p.device)
    ws = _icp_workspace(0, n, p.device)
    check(lib().skimi_estimate_normals(ptr(p), n, float(radius), ptr(normals), ptr(counts), ptr(ws), ws.numel(),
                                       _lib.current_stream()), "skimi_estimate_normals")
    return normals, counts


def icp_correspondences(source: torch.Tensor, target: torch.Tensor, transformation=None, max_distance: float = 0.05):
    """Index of the nearest valid target point at d < max_distance of every source point under `transformation`
    (4x4, default identity) -> int64 [N_src] device tensor, -1 = no correspondence (or invalid source point).
    Ties go to the smaller target index."""
    s, t = _cloud(source, "icp_correspondences"), _cloud(target, "icp_correspondences")
    out = torch.empty((s.shape[0],), dtype=torch.int32, device=s.device)
    ws = _icp_workspace(s.shape[0], t.shape[0], s.device)
    T = _mat4(np.eye(4) if transformation is None else transformation)
    check(lib().skimi_icp_correspondences(ptr(s), s.shape[0], ptr(t), t.shape[0], T, float(max_distance), ptr(out), ptr(ws),
                                          ws.numel(), _lib.current_stream()), "skimi_icp_correspondences")
    return out.to(torch.int64)


@dataclass
class ICPResult:
    """The fields of Open3D's RegistrationResult that the reference reads (transformation) or reports."""
    transformation: np.ndarray   # float64 [4, 4]
    fitness: float               # correspondences / valid source points, last evaluation
    inlier_rmse: float           # sqrt(sum d^2 / correspondences), last evaluation
    iterations: int              # updates applied


def icp_point_to_plane(source: torch.Tensor, target: torch.Tensor, max_correspondence_distance: float = 0.05,
                       normal_radius: float = 0.05, max_iteration: int = 200, relative_fitness: float = 1e-6,
                       relative_rmse: float = 1e-6, init=None) -> ICPResult:
    """registration_icp(source, target, max_correspondence_distance, init, TransformationEstimationPointToPlane(),
    ICPConvergenceCriteria(relative_fitness, relative_rmse, max_iteration)) on device clouds [..., 3], target normals
    from estimate_normals(normal_radius) (multi_view_process.py:487-505).  Fewer than 50 valid points in either cloud:
    identity and 0 iterations (:471-474)."""
    s, t = _cloud(source, "icp_point_to_plane"), _cloud(target, "icp_point_to_plane")
    ws = _icp_workspace(s.shape[0], t.shape[0], s.device)
    T_out = (C.c_double * 16)()
    fit, rmse, iters = C.c_double(), C.c_double(), C.c_int32()
    check(lib().skimi_icp_point_to_plane(ptr(s), s.shape[0], ptr(t), t.shape[0], float(max_correspondence_distance),
                                         float(normal_radius), int(max_iteration), float(relative_fitness), float(relative_rmse),
                                         None if init is None else _mat4(init), T_out, C.byref(fit), C.byref(rmse),
                                         C.byref(iters), ptr(ws), ws.numel(), _lib.current_stream()), "skimi_icp_point_to_plane")
    return ICPResult(np.array(T_out[:], dtype=np.float64).reshape(4, 4), fit.value, rmse.value, iters.value)


# ---- bundle adjustment (run_local_ba of multi_view_process.py:553-564; losses of bundle_adjustment/loss.py) --------
# Rules (DESIGN §2 "BA"): float64 throughout; mode full optimises w [T,C,3] with R = Exp(w) R0 (Rodrigues, Taylor
# branch below theta^2 = 1e-8); the baseline and bone-length means are taken at the current iterate and held
# constant; a clamped Z (< 1e-6) and a zero-length bone or baseline pass no gradient; the two temporal terms are 0 at
# T = 1; Adam with torch's defaults.
BA_MODES = {"pose_only": 0, "pose_cam_t": 1, "full": 2}
# cfg.bundle_adjustment key -> default weight of its loss in bundle_adjustment/loss.py, in the order of the C-ABI
BA_WEIGHT_KEYS = {"ba_weight_reproj": 1.0, "ba_weight_smooth": 1e-2, "ba_weight_baseline": 1e-2,
                  "ba_weight_bone_length": 1e-2, "ba_weight_pose_temporal": 1e-2}
BA_PLACEMENTS = {"auto": 0, "lds": 1, "workspace": 2}


@dataclass
class BAResult:
    mode: str
    R: torch.Tensor          # float64 [T, C, 3, 3]
    t: torch.Tensor          # float64 [T, C, 3]
    X: torch.Tensor          # float64 [T, J, 3]
    history: torch.Tensor    # float64 [num_iters, 6]: total, reprojection, smoothness, baseline, bone length, temporal


def ba_weights(weights=None) -> list:
    """The five loss weights in C-ABI order from a mapping keyed like cfg.bundle_adjustment (absent keys take the
    default `w` of their loss.py function)."""
    weights = dict(weights or {})
    unknown = sorted(set(weights) - set(BA_WEIGHT_KEYS))
    if unknown:
        raise ValueError(f"unknown bundle-adjustment weight keys {unknown}; known: {list(BA_WEIGHT_KEYS)}")
    return [float(weights.get(k, d)) for k, d in BA_WEIGHT_KEYS.items()]


def bundle_adjust(K, R, t, X, x2d, conf, modes=("pose_only",), num_iters: int = 200, lr: float = 1e-3, weights=None,
                  placement: str = "auto") -> list:
    """Bundle adjustment of one clip, every mode in ONE launch (one workgroup per mode): K [C,3,3], R [T,C,3,3],
    t [T,C,3] (world -> camera), X [T,J,3], x2d [T,C,J,2] pixels, conf [T,C,J]; host arrays or device tensors.
    `modes`: a mode name or a sequence of them (pose_only: X; pose_cam_t: X, t; full: X, t, R).  `weights`: a mapping
    with cfg.bundle_adjustment's ba_weight_* keys.  `placement` ("auto", "lds", "workspace"): where the state lives;
    it does not change the results.  -> [BAResult] in the order of `modes`, float64 device tensors."""
    if isinstance(modes, str):
        modes = (modes,)
    modes = list(modes)
    bad = [m for m in modes if m not in BA_MODES]
    if bad or not modes:
        raise ValueError(f"unknown bundle-adjustment modes {bad or modes}; known: {list(BA_MODES)}")
    if placement not in BA_PLACEMENTS:
        raise ValueError(f"unknown placement {placement!r}; known: {list(BA_PLACEMENTS)}")
    w = ba_weights(weights)
    dev = next((a.device for a in (K, R, t, X, x2d, conf) if isinstance(a, torch.Tensor) and a.is_cuda),
               torch.device("cuda", torch.cuda.current_device()))

    def f64(a):
        a = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.asarray(a))
        return a.to(dev, torch.float64).contiguous()

    K, R, t, X, x2d, conf = (f64(a) for a in (K, R, t, X, x2d, conf))
    if X.dim() != 3 or X.shape[-1] != 3:
        raise ValueError(f"bundle_adjust: X must be [T, J, 3], got {tuple(X.shape)}")
    T, J = X.shape[0], X.shape[1]
    Cn = K.shape[0] if K.dim() == 3 else -1
    want = {"K": (Cn, 3, 3), "R": (T, Cn, 3, 3), "t": (T, Cn, 3), "x2d": (T, Cn, J, 2), "conf": (T, Cn, J)}
    for name, a in (("K", K), ("R", R), ("t", t), ("x2d", x2d), ("conf", conf)):
        if tuple(a.shape) != want[name]:
            raise ValueError(f"bundle_adjust: {name} must be {list(want[name])}, got {list(a.shape)}")
    P = len(modes)
    R_out = torch.empty((P, T, Cn, 3, 3), dtype=torch.float64, device=dev)
    t_out = torch.empty((P, T, Cn, 3), dtype=torch.float64, device=dev)
    X_out = torch.empty((P, T, J, 3), dtype=torch.float64, device=dev)
    hist = torch.empty((P, int(num_iters), 6), dtype=torch.float64, device=dev)
    ws = torch.empty(int(lib().skimi_ba_workspace_bytes(T, Cn, J, P)), dtype=torch.uint8, device=dev)
    codes = (C.c_int32 * P)(*[BA_MODES[m] for m in modes])
    check(lib().skimi_bundle_adjust(ptr(K), ptr(R), ptr(t), ptr(X), ptr(x2d), ptr(conf), T, Cn, J, codes, P, int(num_iters),
                                    float(lr), *w, BA_PLACEMENTS[placement], ptr(R_out), ptr(t_out), ptr(X_out),
                                    ptr(hist) if hist.numel() else None, ptr(ws), ws.numel(), _lib.current_stream()),
          "skimi_bundle_adjust")
    return [BAResult(m, R_out[p], t_out[p], X_out[p], hist[p]) for p, m in enumerate(modes)]


# ---- camera resection (VideoPose3D/slove_rt_from_3d.py; rules: DESIGN §2 "Resection") ------------------------------
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
    if not R.is_cuda or not t.is_cuda:
        raise _lib.SkimiError("relative_pose needs device tensors")
    if R.dim() != 4 or tuple(R.shape[2:]) != (3, 3) or tuple(t.shape) != tuple(R.shape[:2]) + (3,):
        raise ValueError(f"relative_pose: need R [G, V, 3, 3] and t [G, V, 3], got {list(R.shape)}, {list(t.shape)}")
    R, t = R.contiguous().to(torch.float64), t.contiguous().to(torch.float64)
    R_rel, t_rel = torch.empty_like(R), torch.empty_like(t)
    check(lib().skimi_relative_pose(ptr(R), ptr(t), R.shape[0], R.shape[1], ptr(R_rel), ptr(t_rel), _lib.current_stream()),
          "skimi_relative_pose")
    return R_rel, t_rel


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
    given = [a for a in (X, x2d, K, conf, R0, t0) if a is not None]
    for a in given:
        if not isinstance(a, torch.Tensor) or not a.is_cuda:
            raise _lib.SkimiError("resect_cameras needs device tensors")
    if loss not in RESECT_LOSSES:
        raise ValueError(f"resect_cameras: unknown loss {loss!r}; known: {list(RESECT_LOSSES)}")
    if X.dim() != 2 or X.shape[1] != 3 or x2d.dim() != 3 or x2d.shape[1:] != (X.shape[0], 2):
        raise ValueError(f"resect_cameras: need X [N, 3] and x2d [V, N, 2], got {list(X.shape)}, {list(x2d.shape)}")
    if (R0 is None) != (t0 is None):
        raise ValueError("resect_cameras: R0 and t0 go together")
    N, V = X.shape[0], x2d.shape[0]
    gs = N if group_size is None else int(group_size)
    G = N // gs if gs >= 1 and N >= 1 else 0
    want = {"K": (V, 3, 3), "conf": (V, N), "R0": (G, V, 3, 3), "t0": (G, V, 3)}
    for name, a in (("K", K), ("conf", conf), ("R0", R0), ("t0", t0)):
        if a is not None and tuple(a.shape) != want[name]:
            raise ValueError(f"resect_cameras: {name} must be {list(want[name])}, got {list(a.shape)}")
    dev = X.device
    X, x2d, K, conf, R0, t0 = (None if a is None else a.to(dev, torch.float64).contiguous() for a in (X, x2d, K, conf, R0, t0))
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)   # noqa: E731
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)     # noqa: E731
    R, t, Ko, c0, c, err, stats = f64(G, V, 3, 3), f64(G, V, 3), f64(G, V, 3, 3), f64(G, V), f64(G, V), f64(V, N), f64(G, V, 3)
    ne, npts, ok = i32(G, V), i32(G, V), i32(G, V)
    nws = int(lib().skimi_resect_workspace_bytes(N, V, gs))
    ws = torch.empty(nws, dtype=torch.uint8, device=dev) if nws else None
    check(lib().skimi_resect_cameras(ptr(X), ptr(x2d), ptr(conf), ptr(K), ptr(R0), ptr(t0), N, V, gs, RESECT_LOSSES[loss],
                                     float(f_scale), float(min_conf), int(max_evals), ptr(R), ptr(t), ptr(Ko), ptr(c0), ptr(c),
                                     ptr(ne), ptr(npts), ptr(ok), ptr(err), ptr(stats), ptr(ws), nws, _lib.current_stream()),
          "skimi_resect_cameras")
    R_rel, t_rel = relative_pose(R, t)
    return ResectResult(R, t, Ko, c0, c, ne, npts, ok.bool(), err, stats[..., 0], stats[..., 1], stats[..., 2], R_rel, t_rel)


# ---- camera-and-points refinement (slove_rt_from_3d.py --refine camera_points; DESIGN §2 "Camera + points refinement") ----
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
    given = [a for a in (X, x2d, K, conf, R0, t0) if a is not None]
    for a in given:
        if not isinstance(a, torch.Tensor) or not a.is_cuda:
            raise _lib.SkimiError("refine_cameras_points needs device tensors")
    if loss not in RESECT_LOSSES:
        raise ValueError(f"refine_cameras_points: unknown loss {loss!r}; known: {list(RESECT_LOSSES)}")
    if X.dim() != 2 or X.shape[1] != 3 or x2d.dim() != 3 or x2d.shape[1:] != (X.shape[0], 2):
        raise ValueError(f"refine_cameras_points: need X [N, 3] and x2d [V, N, 2], got {list(X.shape)}, {list(x2d.shape)}")
    if (R0 is None) != (t0 is None):
        raise ValueError("refine_cameras_points: R0 and t0 go together")
    N, V = X.shape[0], x2d.shape[0]
    gs = N if group_size is None else int(group_size)
    G = N // gs if gs >= 1 and N >= 1 else 0
    want = {"K": (V, 3, 3), "conf": (V, N), "R0": (G, V, 3, 3), "t0": (G, V, 3)}
    for name, a in (("K", K), ("conf", conf), ("R0", R0), ("t0", t0)):
        if a is not None and tuple(a.shape) != want[name]:
            raise ValueError(f"refine_cameras_points: {name} must be {list(want[name])}, got {list(a.shape)}")
    dev = X.device
    X, x2d, K, conf, R0, t0 = (None if a is None else a.to(dev, torch.float64).contiguous() for a in (X, x2d, K, conf, R0, t0))
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)   # noqa: E731
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)     # noqa: E731
    if R0 is None and G >= 1 and 1 <= V <= 4:
        r0 = resect_cameras(X, x2d, K=K, conf=conf, group_size=gs, loss=loss, f_scale=f_scale, min_conf=min_conf, max_evals=1)
        R0, t0 = r0.R, r0.t            # NaN where the resection failed: the group then fails here too
    R, t, Ko, Xo, err, stats = f64(G, V, 3, 3), f64(G, V, 3), f64(G, V, 3, 3), f64(N, 3), f64(V, N), f64(G, V, 3)
    c0, c, moved, ne, npts, ok = f64(G), f64(G), f64(G), i32(G), i32(G), i32(G)
    nws = int(lib().skimi_refine_workspace_bytes(N, V, gs))
    ws = torch.empty(max(nws, 8), dtype=torch.uint8, device=dev)
    check(lib().skimi_refine_cameras_points(ptr(X), ptr(x2d), ptr(conf), ptr(K), ptr(R0), ptr(t0), N, V, gs, float(lambda_x),
                                            RESECT_LOSSES[loss], float(f_scale), float(min_conf), int(max_evals), ptr(R), ptr(t),
                                            ptr(Ko), ptr(Xo), ptr(c0), ptr(c), ptr(ne), ptr(npts), ptr(ok), ptr(err), ptr(stats),
                                            ptr(moved), ptr(ws), nws, _lib.current_stream()),
          "skimi_refine_cameras_points")
    R_rel, t_rel = relative_pose(R, t)
    return RefineResult(R, t, Ko, Xo, c0, c, ne, npts, ok.bool(), err, stats[..., 0], stats[..., 1], stats[..., 2], moved,
                        R_rel, t_rel)


# ---- essential matrix and the pose from it (slove_rt_from_3d.py --init essential, camera_position.py; DESIGN §2 "Essential matrix") ----
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
    for a in (x2d, K, conf):
        if a is not None and (not isinstance(a, torch.Tensor) or not a.is_cuda):
            raise _lib.SkimiError("essential_ransac needs device tensors")
    if x2d.dim() != 3 or x2d.shape[0] != 2 or x2d.shape[2] != 2 or tuple(K.shape) != (2, 3, 3):
        raise ValueError(f"essential_ransac: need x2d [2, N, 2] and K [2, 3, 3], got {list(x2d.shape)}, {list(K.shape)}")
    N = x2d.shape[1]
    if conf is not None and tuple(conf.shape) != (2, N):
        raise ValueError(f"essential_ransac: conf must be {[2, N]}, got {list(conf.shape)}")
    gs = N if group_size is None else int(group_size)
    G = N // gs if gs >= 1 and N >= 1 else 0
    dev = x2d.device
    x2d, K, conf = (None if a is None else a.to(dev, torch.float64).contiguous() for a in (x2d, K, conf))
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)   # noqa: E731
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)     # noqa: E731
    u8 = lambda *shape: torch.empty(shape, dtype=torch.uint8, device=dev)      # noqa: E731
    R, t, E, cost, confd = f64(G, 3, 3), f64(G, 3), f64(G, 3, 3), f64(G), f64(G)
    inl, pm = u8(N), u8(N)
    nu, ni, npose, ch, win, ns, ok = i32(G), i32(G), i32(G), i32(G, 4), i32(G, 2), i32(G), i32(G)
    nws = int(lib().skimi_essential_workspace_bytes(N, gs, int(hypotheses)))
    ws = torch.empty(max(nws, 8), dtype=torch.uint8, device=dev)
    check(lib().skimi_essential_ransac(ptr(x2d), ptr(conf), ptr(K), N, gs, float(min_conf), float(threshold), int(hypotheses),
                                       int(seed) & 0xFFFFFFFFFFFFFFFF, int(group_offset), float(baseline), float(distance_thresh),
                                       ptr(R), ptr(t), ptr(E), ptr(inl), ptr(pm), ptr(nu), ptr(ni), ptr(npose), ptr(ch), ptr(cost),
                                       ptr(win), ptr(ns), ptr(confd), ptr(ok), ptr(ws), nws, _lib.current_stream()),
          "skimi_essential_ransac")
    return EssentialResult(R, t, E, inl, pm, nu, ni, npose, ch, cost, win, ns, confd, ok.bool())


def five_point(a: torch.Tensor, b: torch.Tensor):
    """The five-point solver alone, one thread per sample: a, b [S, 5, 2] normalised coordinates (float64, device) -> (E
    [S, 10, 3, 3] with b^T E a = 0, ||E||_F = sqrt 2, a sample's solutions by x ascending and NaN beyond its count,
    counts [S] int32).  DESIGN §2 "Essential matrix", rule 4."""
    if not (isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor) and a.is_cuda and b.is_cuda):
        raise _lib.SkimiError("five_point needs device tensors")
    if a.dim() != 3 or tuple(a.shape[1:]) != (5, 2) or a.shape != b.shape:
        raise ValueError(f"five_point: need a, b [S, 5, 2], got {list(a.shape)}, {list(b.shape)}")
    a, b = a.to(torch.float64).contiguous(), b.to(torch.float64).contiguous()
    S = a.shape[0]
    E = torch.empty((S, 10, 3, 3), dtype=torch.float64, device=a.device)
    counts = torch.empty((S,), dtype=torch.int32, device=a.device)
    check(lib().skimi_five_point(ptr(a), ptr(b), S, ptr(E), ptr(counts), _lib.current_stream()), "skimi_five_point")
    return E, counts


# ---- fusion + temporal smoothing (fuse.py on the device; rules: DESIGN §2 "Fusion + smoothing on the device") --------------
FUSE_MAX_JOINTS = 128
FUSE_SCALE_MODES = {"hip": 0, "torso": 1}
SAVGOL_MAX_WIN = 33


class FuseH36MResult(NamedTuple):
    """fuse_h36m's outputs (device tensors; T frames)."""
    fused: torch.Tensor       # float64 [T, 17, 3]: pelvis at the origin, pelvis-neck distance 1; NaN for a status-0 frame
    R: torch.Tensor           # float64 [T, 3, 3]
    t: torch.Tensor           # float64 [T, 3]
    s: torch.Tensor           # float64 [T]
    diag: torch.Tensor        # float64 [T, 4]: FUSE_DIAG_FIELDS
    status: torch.Tensor      # bool [T]: False where fewer than 3 torso joints are finite on both sides (the host raises)
    mean_gain: torch.Tensor   # float64 []: nanmean of the gains (NaN for T = 0)
    bad_frames: torch.Tensor  # bool [T]: gain < 0


FUSE_DIAG_FIELDS = ("LR_before", "Fused_vs_L", "Fused_vs_R", "gain")


class FuseViewsResult(NamedTuple):
    """fuse_views' outputs (device tensors; T frames, J joints)."""
    fused: torch.Tensor       # float64 [T, J, 3]
    aligned: torch.Tensor     # float64 [T, J, 3]: the right view in the left view's frame
    q_l: torch.Tensor         # float64 [T, J] = sqrt(conf_l conf_x)
    q_r: torch.Tensor
    conf_l: torch.Tensor      # float64 [T, J]: weak-perspective reprojection confidence of the view's raw 3D
    conf_r: torch.Tensor
    conf_x: torch.Tensor      # float64 [T, J]: cross-view consistency confidence
    err_l: torch.Tensor       # float64 [T, J]: the reprojection residual in pixels, NaN where undefined
    err_r: torch.Tensor
    dist: torch.Tensor        # float64 [T, J]: distance of the two canonical poses, NaN where undefined
    fit_ok: torch.Tensor      # bool [T, 2]: the (left, right) weak-perspective fit exists (the host raises where it does not)


class EmaResult(NamedTuple):
    """smooth_ema's outputs (device tensors)."""
    X: torch.Tensor           # float64 [T, J, 3]
    base: torch.Tensor        # float64 [J]: the per-joint base factor the kernel ran with


class SavgolResult(NamedTuple):
    """smooth_savgol's outputs."""
    X: torch.Tensor           # float64 [T, J, 3] (device)
    window: int               # the window used (the reference's quirk: 3 for every odd T)


def _f64_dev(name, a, dev=None):
    if not isinstance(a, torch.Tensor) or not a.is_cuda:
        raise _lib.SkimiError(f"{name} needs device tensors")
    return a.to(a.device if dev is None else dev, torch.float64).contiguous()


def fuse_h36m(left_3d: torch.Tensor, right_3d: torch.Tensor, tau=0.08, allow_scale: bool = False, mirror_right_x: bool = False,
              wL=None, wR=None) -> FuseH36MResult:
    """fuse.fuse_pose_no_extrinsics_h36m for a whole clip in one launch: left_3d, right_3d [T, 17, 3] (or [17, 3]) device
    tensors; tau a number or [17]; wL, wR None, [17] or [T, 17] -> FuseH36MResult.  Where the host raises ValueError (fewer
    than 3 torso joints finite on both sides) the frame is NaN and its status False.  mean_gain and bad_frames are torch
    ops on the device: nothing is read back."""
    L, R = _f64_dev("fuse_h36m", left_3d), _f64_dev("fuse_h36m", right_3d)
    if L.dim() == 2:
        L = L[None]
    if R.dim() == 2:
        R = R[None]
    if L.shape != R.shape or L.dim() != 3 or tuple(L.shape[1:]) != (17, 3):
        raise ValueError(f"fuse_h36m: inputs must both be (*, 17, 3), got {list(L.shape)}, {list(R.shape)}")
    T, dev = L.shape[0], L.device
    tau_j = None
    if isinstance(tau, (float, int)):
        tau_s = float(tau)
    else:
        tau_s = 0.0
        tau_j = (tau if isinstance(tau, torch.Tensor) else torch.as_tensor(np.asarray(tau, dtype=np.float64))).to(dev, torch.float64).contiguous()
        if tuple(tau_j.shape) != (17,):
            raise ValueError(f"fuse_h36m: tau must be a number or [17], got {list(tau_j.shape)}")

    def weights(w, name):
        if w is None:
            return None, 0
        w = (w if isinstance(w, torch.Tensor) else torch.as_tensor(np.asarray(w, dtype=np.float64))).to(dev, torch.float64).contiguous()
        if tuple(w.shape) not in ((17,), (T, 17)):
            raise ValueError(f"fuse_h36m: {name} must be [17] or [{T}, 17], got {list(w.shape)}")
        return w, 17 if w.dim() == 2 else 0

    (wl, sl), (wr, sr) = weights(wL, "wL"), weights(wR, "wR")
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)   # noqa: E731
    fused, Rm, tv, s, diag = f64(T, 17, 3), f64(T, 3, 3), f64(T, 3), f64(T), f64(T, 4)
    status = torch.empty((T,), dtype=torch.int32, device=dev)
    check(lib().skimi_fuse_h36m(ptr(L), ptr(R), T, tau_s, ptr(tau_j), ptr(wl), sl, ptr(wr), sr, int(bool(allow_scale)),
                                int(bool(mirror_right_x)), ptr(fused), ptr(Rm), ptr(tv), ptr(s), ptr(diag), ptr(status),
                                _lib.current_stream()), "skimi_fuse_h36m")
    gain = diag[:, 3]
    return FuseH36MResult(fused, Rm, tv, s, diag, status.bool(), torch.nanmean(gain) if T else gain.new_full((), float("nan")),
                          gain < 0)


def fuse_views(X_l: torch.Tensor, X_r: torch.Tensor, U_l: torch.Tensor, U_r: torch.Tensor, *, root_idx: int, left_hip_idx: int,
               right_hip_idx: int, left_shoulder_idx: int, right_shoulder_idx: int, sigma_px: float = 12.0, sigma_3d: float = 0.08,
               scale_mode: str = "hip", min_points: int = 8) -> FuseViewsResult:
    """The per-frame body of fuse/main_raw.py for a whole clip in one launch: X_l, X_r [T, J, 3] the two views' 3D joints,
    U_l, U_r [T, J, 2] their 2D keypoints (NaN = missing), device tensors, J <= 128 -> FuseViewsResult: fuse.
    align_right_to_left, fuse.weakpersp_reproj_confidence of each view on its raw 3D, fuse.crossview_consistency_confidence
    of the raw pair, q = sqrt(conf conf_x), fuse.fuse_frame_3d(X_l, aligned, q_l, q_r).  Where the host's weak-perspective
    fit raises (fewer than min_points rows, no spread) the view's conf is 0, its err NaN and its fit_ok False."""
    Xl, Xr, Ul, Ur = (_f64_dev("fuse_views", a) for a in (X_l, X_r, U_l, U_r))
    if scale_mode not in FUSE_SCALE_MODES:
        raise ValueError("scale_mode must be 'hip' or 'torso'")
    if Xl.dim() != 3 or Xl.shape[2] != 3 or Xr.shape != Xl.shape or tuple(Ul.shape) != (*Xl.shape[:2], 2) or Ur.shape != Ul.shape:
        raise ValueError(f"fuse_views: need X_l, X_r [T, J, 3] and U_l, U_r [T, J, 2], got {list(Xl.shape)}, {list(Xr.shape)}, "
                         f"{list(Ul.shape)}, {list(Ur.shape)}")
    T, J, dev = Xl.shape[0], Xl.shape[1], Xl.device
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)   # noqa: E731
    fused, aligned = f64(T, J, 3), f64(T, J, 3)
    per_joint = [f64(T, J) for _ in range(8)]
    fit_ok = torch.empty((T, 2), dtype=torch.int32, device=dev)
    check(lib().skimi_fuse_views(ptr(Xl), ptr(Xr), ptr(Ul), ptr(Ur), T, J, int(root_idx), int(left_hip_idx), int(right_hip_idx),
                                 int(left_shoulder_idx), int(right_shoulder_idx), float(sigma_px), float(sigma_3d),
                                 FUSE_SCALE_MODES[scale_mode], int(min_points), ptr(fused), ptr(aligned), *map(ptr, per_joint),
                                 ptr(fit_ok), _lib.current_stream()), "skimi_fuse_views")
    return FuseViewsResult(fused, aligned, *per_joint, fit_ok.bool())


def smooth_ema(X: torch.Tensor, target_ids=None, alpha: float = 0.7, adaptive: bool = True, alpha_min: float = 0.45,
               alpha_max: float = 0.92, speed_gain: float = 0.25) -> EmaResult:
    """fuse.temporal_smooth_ema on the device: X [T, J, 3] (NaN rows = missing joints) -> EmaResult.  One thread per joint
    walks the clip; the per-joint base factors come from alpha, target_ids and fuse._ALPHA_FACTOR as on the host."""
    from . import fuse

    X = _f64_dev("smooth_ema", X)
    if X.dim() != 3 or X.shape[2] != 3:
        raise ValueError(f"smooth_ema: need X [T, J, 3], got {list(X.shape)}")
    T, J = X.shape[:2]
    if adaptive:
        ids = np.arange(J) if target_ids is None else np.asarray(list(target_ids), dtype=np.int64)
        if ids.shape != (J,):
            raise ValueError(f"smooth_ema: {ids.size} target_ids for {J} joints")
        known = (ids >= 0) & (ids < fuse._ALPHA_FACTOR.size)
        factor = np.where(known, fuse._ALPHA_FACTOR[np.where(known, ids, 0)], 1.0)
        base = np.clip(float(alpha) * factor, alpha_min, alpha_max)
    else:
        base = np.full(J, float(alpha))
    base = torch.from_numpy(np.ascontiguousarray(base, dtype=np.float64)).to(X.device)
    Y = torch.empty_like(X)
    check(lib().skimi_smooth_ema(ptr(X), T, J, ptr(base), int(bool(adaptive)), float(alpha_min), float(alpha_max),
                                 float(speed_gain), ptr(Y), _lib.current_stream()), "skimi_smooth_ema")
    return EmaResult(Y, base)


_savgol_ops = {}   # (win, poly, device) -> the three operators on the device


def smooth_savgol(X: torch.Tensor, win: int = 9, poly: int = 2) -> SavgolResult:
    """fuse.smooth_skeleton on the device: X [T, J, 3] -> SavgolResult.  The window is the reference's min(odd(win), max(1
    if T is odd else T - 1, 3)); every (joint, coordinate) series with at least that many finite samples is filtered over
    them as one contiguous series, everything else passes through bit for bit.  The window must not exceed 33 and must
    exceed poly (the host raises for poly >= window only once a series is long enough to be filtered)."""
    from . import fuse

    X = _f64_dev("smooth_savgol", X)
    if X.dim() != 3 or X.shape[2] != 3:
        raise ValueError(f"smooth_savgol: need X [T, J, 3], got {list(X.shape)}")
    T, J = X.shape[:2]
    w = fuse.savgol_window(T, int(win))
    Y = torch.empty_like(X)
    key = (w, int(poly), X.device)
    if key not in _savgol_ops and 1 <= w <= SAVGOL_MAX_WIN and 0 <= int(poly) < w:
        _savgol_ops[key] = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(X.device) for a in fuse.savgol_operators(w, int(poly)))
    fir, first, last = _savgol_ops.get(key, (None, None, None))     # a refused (win, poly) has none: the library says why
    check(lib().skimi_smooth_savgol(ptr(X), T, J, w, int(poly), ptr(fir), ptr(first), ptr(last), ptr(Y), _lib.current_stream()),
          "skimi_smooth_savgol")
    return SavgolResult(Y, w)


# ---- kinematic analysis of clips: angle/main.py (csrc/kinematics.hip; rules: include/skimi.h, DESIGN §2 "Kinematics") ------
KIN_ROLES = ("shoulder_l", "shoulder_r", "elbow_l", "elbow_r", "hip_l", "hip_r", "knee_l", "knee_r", "foot_l", "foot_r",
             "hand_l", "hand_r", "neck")
KIN_BASE_SERIES = ("knee_l", "knee_r", "elbow_l", "elbow_r", "shoulder_l", "shoulder_r", "hip_l", "hip_r", "torso_knee_angle",
                   "knee_diff_lr", "elbow_distance_l", "elbow_distance_r", "tilt_upper", "tilt_lower")
KIN_SERIES = KIN_BASE_SERIES + tuple(n + s for n in KIN_BASE_SERIES for s in ("_d", "_abs_d"))      # the 42, in order
KIN_STAT_FIELDS = ("mean", "std", "min", "max")
# the joint of each role (KIN_ROLES order) among the reference's 15 joints: MHR-70 ids 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 62,
# 41, 69 as positions in its TARGET_IDS order (1, 2, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 41, 62, 69)
KIN_LAYOUT_MHR70_15 = (2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 12, 14)
KIN_LDS_FRAMES = 2048       # SKIMI_KIN_LDS_FRAMES: longer clips keep their arrays in a workspace


class KinematicsResult(NamedTuple):
    """kinematics' outputs (device tensors; B clips, T frames, M = kin_max_turns(T, min_turn_frames) turn slots).  Frames at
    and beyond a clip's length: NaN series, changes, heading, heading_smooth and velocity_smooth, boundary False.  Turn slots
    at and beyond n_turns: turn_frames, turn_direction and turn_counts 0; turn_heading_change and turn_stats NaN."""
    series: torch.Tensor                # float64 [B, 14, T]: KIN_BASE_SERIES
    changes: torch.Tensor               # float64 [B, 28, T]: name_d, name_abs_d of each base series (KIN_SERIES[14:])
    heading: torch.Tensor               # float64 [B, T] degrees
    heading_smooth: torch.Tensor        # float64 [B, T]: filled, unwrapped, box mean; NaN with fewer than 5 finite headings
    velocity_smooth: torch.Tensor       # float64 [B, T]
    boundary: torch.Tensor              # bool [B, T]: first and last frame of every kept turn
    n_turns: torch.Tensor               # int32 [B]
    turn_frames: torch.Tensor           # int32 [B, M, 2]: (start, end), inclusive
    turn_heading_change: torch.Tensor   # float64 [B, M]
    turn_direction: torch.Tensor        # int32 [B, M]: +1 (heading change > 0) or -1
    turn_stats: torch.Tensor            # float64 [B, M, 42, 4]: KIN_STAT_FIELDS of KIN_SERIES over the turn's finite samples
    turn_counts: torch.Tensor           # int32 [B, M, 42]: the number of those samples
    all_series: torch.Tensor            # float64 [B, 42, T]: the storage `series` and `changes` are views of


def kin_max_turns(frames: int, min_turn_frames: int = 12) -> int:
    """The most turns a clip of `frames` frames can hold: boundaries after frame 0 are at least min_turn_frames apart, so at
    most (frames - 1) // min_turn_frames extrema are taken, and the last frame closes at most one more segment."""
    return (int(frames) - 1) // int(min_turn_frames) + 1 if frames > 0 and min_turn_frames >= 1 else 0


def kinematics(X: torch.Tensor, lengths=None, layout=KIN_LAYOUT_MHR70_15, up_axis=(0.0, -1.0, 0.0), min_turn_frames: int = 12,
               min_heading_change_deg: float = 8.0, heading_window: int = 11, velocity_window: int = 9, *,
               placement: str = "auto") -> KinematicsResult:
    """angle/main.py's _compute_all_series, compute_series_changes, detect_turn_segments and the statistics of
    save_turn_reports for a batch of clips in three launches: X [B, T, J, 3] (a [T, J, 3] input is one clip) device tensor;
    lengths None or [B] integers, 0 <= length <= T (the frames beyond a clip's length are never read); layout the joint index
    of each role in KIN_ROLES order, -1 for absent -> KinematicsResult.  Nothing is read back: the turn count stays on the
    device.  placement "auto" keeps a clip's arrays in LDS up to KIN_LDS_FRAMES frames and in a workspace beyond; "workspace"
    forces the workspace (same bits)."""
    X = _f64_dev("kinematics", X)
    if X.dim() == 3:
        X = X[None]
    if X.dim() != 4 or X.shape[3] != 3:
        raise ValueError(f"kinematics: need X [B, T, J, 3] or [T, J, 3], got {list(X.shape)}")
    if placement not in ("auto", "workspace"):
        raise ValueError("placement must be 'auto' or 'workspace'")
    B, T, J = (int(s) for s in X.shape[:3])
    dev = X.device
    lay = np.asarray(list(layout), dtype=np.int64)
    if lay.shape != (len(KIN_ROLES),):
        raise ValueError(f"kinematics: layout needs {len(KIN_ROLES)} joint indices ({', '.join(KIN_ROLES)}), got {lay.size}")
    lay_c = (C.c_int32 * len(KIN_ROLES))(*[int(np.clip(v, -2 ** 31, 2 ** 31 - 1)) for v in lay])
    up = np.asarray(up_axis, dtype=np.float64)
    if up.shape != (3,):
        raise ValueError(f"kinematics: up_axis must be [3], got {list(up.shape)}")
    up_c = (C.c_double * 3)(*up.tolist())
    len_t = None
    if lengths is not None:
        len_t = (lengths if isinstance(lengths, torch.Tensor) else torch.as_tensor(np.asarray(lengths, dtype=np.int64)))
        if tuple(len_t.shape) != (B,):
            raise ValueError(f"kinematics: lengths must be [{B}], got {list(len_t.shape)}")
        len_t = len_t.to(dev, torch.int32).contiguous()
    M = kin_max_turns(T, min_turn_frames)
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)   # noqa: E731
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)     # noqa: E731
    alls, heading, hs, vs = f64(B, len(KIN_SERIES), T), f64(B, T), f64(B, T), f64(B, T)
    boundary = torch.empty((B, T), dtype=torch.uint8, device=dev)
    n_turns, frames, dh, direction = i32(B), i32(B, M, 2), f64(B, M), i32(B, M)
    stats, counts = f64(B, M, len(KIN_SERIES), 4), i32(B, M, len(KIN_SERIES))
    ws, ws_bytes = None, 0
    if placement == "workspace" or T > KIN_LDS_FRAMES:
        ws_bytes = int(lib().skimi_kin_workspace_bytes(B, T))
        ws = torch.empty((max(ws_bytes, 8) // 8,), dtype=torch.float64, device=dev) if B and T else None
    check(lib().skimi_kinematics(ptr(X), ptr(len_t), B, T, J, lay_c, up_c, int(min_turn_frames), float(min_heading_change_deg),
                                 int(heading_window), int(velocity_window), M, ptr(ws), ws_bytes, ptr(alls), ptr(heading), ptr(hs),
                                 ptr(vs), ptr(boundary), ptr(n_turns), ptr(frames), ptr(dh), ptr(direction), ptr(stats),
                                 ptr(counts), _lib.current_stream()), "skimi_kinematics")
    nb = len(KIN_BASE_SERIES)
    return KinematicsResult(alls[:, :nb], alls[:, nb:], heading, hs, vs, boundary.bool(), n_turns, frames, dh, direction, stats,
                            counts, alls)


# ---- pose evaluation of clips (csrc/evaluate.hip; rules: include/skimi.h, DESIGN §2 "Evaluation") -------------------------
EVAL_MAX_JOINTS, EVAL_MAX_EDGES, EVAL_MAX_PAIRS = 128, 128, 64
EVAL_LDS_ELEMS = 1440       # SKIMI_EVAL_LDS_ELEMS: clips with more frames * joints keep their arrays in a workspace
JOINT_STAT_FIELDS = ("mean", "std", "median")
# VideoPose3D/fuse/fuse_eval.py:21-42, the Human3.6M skeleton: bones, the (left, right) joint pairs, each side's bones
H36M_EDGES = ((0, 1), (1, 2), (2, 3), (0, 4), (4, 5), (5, 6), (0, 7), (7, 8), (8, 9), (9, 10), (8, 11), (11, 12), (12, 13), (8, 14),
              (14, 15), (15, 16))
H36M_LR_PAIRS = ((4, 1), (5, 2), (6, 3), (14, 11), (15, 12), (16, 13))
H36M_LEFT_BONES = ((0, 4), (4, 5), (5, 6), (8, 14), (14, 15), (15, 16))
H36M_RIGHT_BONES = ((0, 1), (1, 2), (2, 3), (8, 11), (11, 12), (12, 13))
# metrics/true_data_compare.py:66-81 BONE_EDGES (MHR-70 ids (69, 5), (5, 7), (7, 62), (69, 6), (6, 8), (8, 41), (69, 9), (9, 11),
# (11, 13), (69, 10), (10, 12), (12, 14), (9, 10), (5, 6)) as positions in its TARGET_IDS order (1, 2, 5, 6, 7, 8, 9, 10, 11, 12,
# 13, 14, 41, 62, 69), with the sides and pairs that follow from them
MHR70_15_EDGES = ((14, 2), (2, 4), (4, 13), (14, 3), (3, 5), (5, 12), (14, 6), (6, 8), (8, 10), (14, 7), (7, 9), (9, 11), (6, 7), (2, 3))
MHR70_15_LEFT_BONES = ((14, 2), (2, 4), (4, 13), (14, 6), (6, 8), (8, 10))
MHR70_15_RIGHT_BONES = ((14, 3), (3, 5), (5, 12), (14, 7), (7, 9), (9, 11))
MHR70_15_LR_PAIRS = ((0, 1), (2, 3), (4, 5), (6, 7), (8, 9), (10, 11), (13, 12))


class PoseErrorsResult(NamedTuple):
    """pose_errors' outputs (device tensors; B clips, T frames, J joints).  Frames at and beyond a clip's length: every float
    NaN, n_valid_f 0, p_status False."""
    err: torch.Tensor           # float64 [B, T, J]: ||pred - target|| on valid joints, NaN elsewhere
    p_err: torch.Tensor         # float64 [B, T, J]: the same after the frame's Procrustes alignment; NaN where p_status is False
    vel_err: torch.Tensor       # float64 [B, T, J]: the velocity error against the frame before; row 0 NaN
    mpjpe_f: torch.Tensor       # float64 [B, T]: the mean of the frame's finite err
    n_mpjpe_f: torch.Tensor     # float64 [B, T]: complete frames only
    p_mpjpe_f: torch.Tensor     # float64 [B, T]: complete frames only
    n_valid_f: torch.Tensor     # int32 [B, T]: the frame's valid joints (J = a complete frame)
    p_status: torch.Tensor      # bool [B, T]: the Procrustes alignment exists (the reference raises or returns NaN where not)
    aligned: torch.Tensor       # float64 [B, T, J, 3] = scale * pred @ R + t, or None unless aligned=True
    p_R: torch.Tensor           # float64 [B, T, 3, 3] or None
    p_scale: torch.Tensor       # float64 [B, T] or None
    p_t: torch.Tensor           # float64 [B, T, 3] or None
    mpjpe: torch.Tensor         # float64 [B]: the mean over the clip's finite err
    p_mpjpe: torch.Tensor       # float64 [B]: the mean of p_mpjpe_f over the frames that have one
    n_mpjpe: torch.Tensor       # float64 [B]
    mpjve: torch.Tensor         # float64 [B]: the mean over the clip's finite vel_err
    n_err: torch.Tensor         # int32 [B]: the number of finite err
    n_complete: torch.Tensor    # int32 [B]: the number of complete frames
    n_vel: torch.Tensor         # int32 [B]: the number of finite vel_err
    joint_err: torch.Tensor     # float64 [B, J, 3]: JOINT_STAT_FIELDS of each joint's finite err over the clip
    joint_err_n: torch.Tensor   # int32 [B, J]: their number (0: three NaN)
    joint_p_err: torch.Tensor   # float64 [B, J, 3]: the same of p_err
    joint_p_err_n: torch.Tensor
    metrics: torch.Tensor       # float64 [B, 4]: the storage of mpjpe, p_mpjpe, n_mpjpe, mpjve, in that order


class ClipQualityResult(NamedTuple):
    """clip_quality's outputs (device tensors; B clips, T frames, E edges)."""
    bone_cv_pooled: torch.Tensor       # float64 [B]: nanstd / (nanmean + 1e-9) of all bone lengths (fuse_eval's "Bone Length CV")
    bone_cv_mean: torch.Tensor         # float64 [B]: the mean of bone_cv_edge over the edges that have one (compute_bone_length_cv)
    lr_length_symmetry: torch.Tensor   # float64 [B]
    speed_mean: torch.Tensor           # float64 [B]: NaN with fewer than 3 frames
    jerk_mean: torch.Tensor            # float64 [B]
    speed_p95: torch.Tensor            # float64 [B]: NaN with fewer than 3 frames (the reference leaves the key out)
    accel_p95: torch.Tensor            # float64 [B]
    mirror_symmetry: torch.Tensor      # float64 [B]: of the clip's last frame
    bone_cv_edge: torch.Tensor         # float64 [B, E]
    bone_len: torch.Tensor             # float64 [B, T, E]: NaN where an endpoint is not finite and beyond the clip's length
    scalars: torch.Tensor              # float64 [B, 8]: the storage of the eight per-clip figures, in the order above


def _clips(name, X, dev=None):
    X = _f64_dev(name, X, dev)
    if X.dim() == 3:
        X = X[None]
    if X.dim() != 4 or X.shape[3] != 3:
        raise ValueError(f"{name}: need [B, T, J, 3] or [T, J, 3], got {list(X.shape)}")
    return X


def _lengths(name, lengths, B, dev):
    if lengths is None:
        return None
    len_t = lengths if isinstance(lengths, torch.Tensor) else torch.as_tensor(np.asarray(lengths, dtype=np.int64))
    if tuple(len_t.shape) != (B,):
        raise ValueError(f"{name}: lengths must be [{B}], got {list(len_t.shape)}")
    return len_t.to(dev, torch.int32).contiguous()


def _index_list(name, what, pairs, limit):
    a = np.asarray(list(pairs), dtype=np.int64).reshape(-1, 2) if len(pairs) else np.zeros((0, 2), dtype=np.int64)
    if a.shape[0] > limit:
        raise ValueError(f"{name}: {a.shape[0]} {what}, at most {limit}")
    flat = [int(np.clip(v, -2 ** 31, 2 ** 31 - 1)) for v in a.reshape(-1)]
    return (C.c_int32 * max(len(flat), 1))(*flat), a.shape[0]


def pose_errors(pred: torch.Tensor, target: torch.Tensor, lengths=None, zero_root=None, aligned: bool = False) -> PoseErrorsResult:
    """The MPJPE protocols of VideoPose3D/common/loss.py (mpjpe, p_mpjpe, n_mpjpe, mean_velocity_error) and the per-joint
    tables of metrics/unity_data_compare.py for a batch of (prediction, target) clips in three launches: pred, target
    [B, T, J, 3] (a [T, J, 3] input is one clip) device tensors, J <= 128; lengths None or [B] integers, 0 <= length <= T (the
    frames beyond a clip's length are never read); zero_root None or a joint index: that joint of the target counts as (0, 0,
    0), evaluate()'s `inputs_3d[:, :, 0] = 0`, and the input is not written -> PoseErrorsResult.  aligned=True also returns
    the aligned prediction with its rotation, scale and translation.  Nothing is read back."""
    P, G = _clips("pose_errors", pred), _clips("pose_errors", target)
    if P.shape != G.shape:
        raise ValueError(f"pose_errors: pred {list(P.shape)} and target {list(G.shape)} differ")
    if G.device != P.device:
        raise ValueError("pose_errors: pred and target live on different devices")
    B, T, J = (int(s) for s in P.shape[:3])
    dev = P.device
    len_t = _lengths("pose_errors", lengths, B, dev)
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)   # noqa: E731
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)     # noqa: E731
    err, p_err, vel = f64(B, T, J), f64(B, T, J), f64(B, T, J)
    mf, nf, pf, nv, st = f64(B, T), f64(B, T), f64(B, T), i32(B, T), i32(B, T)
    al, pR, ps, pt = (f64(B, T, J, 3), f64(B, T, 3, 3), f64(B, T), f64(B, T, 3)) if aligned else (None,) * 4
    metrics, counts, jstats, jn = f64(B, 4), i32(B, 3), f64(B, 2, J, 3), i32(B, 2, J)
    check(lib().skimi_pose_errors(ptr(P), ptr(G), ptr(len_t), B, T, J, -1 if zero_root is None else int(zero_root), ptr(err), ptr(p_err),
                                  ptr(vel), ptr(mf), ptr(nf), ptr(pf), ptr(nv), ptr(st), ptr(al), ptr(pR), ptr(ps), ptr(pt), ptr(metrics),
                                  ptr(counts), ptr(jstats), ptr(jn), _lib.current_stream()), "skimi_pose_errors")
    return PoseErrorsResult(err, p_err, vel, mf, nf, pf, nv, st.bool(), al, pR, ps, pt, metrics[:, 0], metrics[:, 1], metrics[:, 2],
                            metrics[:, 3], counts[:, 0], counts[:, 1], counts[:, 2], jstats[:, 0], jn[:, 0], jstats[:, 1], jn[:, 1],
                            metrics)


def clip_quality(X: torch.Tensor, lengths=None, edges=H36M_EDGES, left_edges=H36M_LEFT_BONES, right_edges=H36M_RIGHT_BONES,
                 lr_pairs=H36M_LR_PAIRS, *, placement: str = "auto") -> ClipQualityResult:
    """The ground-truth-free figures of VideoPose3D/fuse/fuse_eval.py (bone-length CV, left/right length symmetry, Speed /
    Accel P95, mirror symmetry) and metrics/true_data_compare.py (speed and jerk means, the per-edge bone CV) for a batch of
    clips in one launch: X [B, T, J, 3] (a [T, J, 3] input is one clip) device tensor, J <= 128; lengths as in pose_errors;
    edges, left_edges, right_edges lists of joint pairs (at most 128 each), lr_pairs (left, right) joints (at most 64): the
    defaults are the reference's Human3.6M lists, MHR70_15_* those of its 15-joint layout -> ClipQualityResult.  placement
    "auto" keeps a clip's arrays in LDS up to T * J = EVAL_LDS_ELEMS and in a workspace beyond; "workspace" forces the
    workspace (same bits).  Nothing is read back."""
    X = _clips("clip_quality", X)
    if placement not in ("auto", "workspace"):
        raise ValueError("placement must be 'auto' or 'workspace'")
    B, T, J = (int(s) for s in X.shape[:3])
    dev = X.device
    len_t = _lengths("clip_quality", lengths, B, dev)
    (e_c, E), (l_c, EL), (r_c, ER) = (_index_list("clip_quality", w, v, EVAL_MAX_EDGES) for w, v in
                                      (("edges", edges), ("left_edges", left_edges), ("right_edges", right_edges)))
    p_c, NP = _index_list("clip_quality", "lr_pairs", lr_pairs, EVAL_MAX_PAIRS)
    scalars = torch.empty((B, 8), dtype=torch.float64, device=dev)
    cv_edge = torch.empty((B, E), dtype=torch.float64, device=dev)
    bone_len = torch.empty((B, T, E), dtype=torch.float64, device=dev)
    ws, ws_bytes = None, 0
    if placement == "workspace" or T * J > EVAL_LDS_ELEMS:
        ws_bytes = int(lib().skimi_eval_workspace_bytes(B, T, J))
        ws = torch.empty((max(ws_bytes, 8) // 8,), dtype=torch.float64, device=dev) if B and T else None
    check(lib().skimi_clip_quality(ptr(X), ptr(len_t), B, T, J, e_c, E, l_c, EL, r_c, ER, p_c, NP, ptr(ws), ws_bytes, ptr(scalars),
                                   ptr(cv_edge), ptr(bone_len), _lib.current_stream()), "skimi_clip_quality")
    return ClipQualityResult(*(scalars[:, k] for k in range(8)), cv_edge, bone_len, scalars)


# ---- lens distortion of points (csrc/lens.hip; rules: include/skimi.h, DESIGN §2 "Lens distortion") -----------------------
# OpenCV's rational + tangential + thin-prism model.  Calibrations are small HOST arrays (NumPy, lists or CPU tensors; a
# device tensor is copied back): they reach the kernels by value.  Batch rule of the three point functions: K [3, 3] is
# one camera for every point of x [..., 2]; K [C, 3, 3] is one camera per entry of the axis before the points' own,
# x [..., C, n, 2], and everything in front of that axis is batch (keypoints [T, V, J, 2] with a calibration per view:
# one launch).  dist is [k] (shared) or [C, k], k in LENS_COEFF_COUNTS.
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


def _host_f64(a) -> np.ndarray:
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64))


def lens_coeffs(dist) -> np.ndarray:
    """OpenCV coefficient vectors [..., k], k = 4, 5, 8, 12 or 14 in cv2's order (k1 k2 p1 p2 k3 k4 k5 k6 s1 s2 s3 s4 tx ty) ->
    float64 [..., 12], zero-padded.  None: twelve zeros.  Non-zero tx / ty (the tilt model) is refused."""
    if dist is None:
        return np.zeros(12, np.float64)
    d = _host_f64(dist)
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


def _lens_matrix(name, what, M, C):
    """[3, 3] or [C, 3, 3] host matrix -> float64 [C or 1, 3, 3]; only fx, fy, cx, cy are part of the model"""
    M = _host_f64(M)
    if M.shape[-2:] != (3, 3) or M.ndim not in (2, 3):
        raise ValueError(f"{name}: {what} must be [3, 3] or [C, 3, 3], got {list(M.shape)}")
    M = M.reshape(-1, 3, 3)
    if C is not None and M.shape[0] != C:
        if M.shape[0] != 1:
            raise ValueError(f"{name}: {what} holds {M.shape[0]} cameras, K holds {C}")
        M = np.ascontiguousarray(np.broadcast_to(M, (C, 3, 3)))
    if not (np.isfinite(M[:, [0, 1, 0, 1], [0, 1, 2, 2]]).all() and (M[:, 0, 0] != 0).all() and (M[:, 1, 1] != 0).all()):
        raise ValueError(f"{name}: {what} needs finite, non-zero focal lengths and a finite principal point")
    return M


def _lens_setup(name, x, K, dist, last):
    """-> (K [C, 3, 3], dist [C, 12], per_camera, outer, C, n) for points x [..., last] under the batch rule above"""
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise _lib.SkimiError(f"{name} needs a device tensor of points")
    if x.dim() < 1 or x.shape[-1] != last:
        raise ValueError(f"{name}: points must be [..., {last}], got {list(x.shape)}")
    per_camera = _host_f64(K).ndim == 3
    Kh = _lens_matrix(name, "K", K, None)
    C = Kh.shape[0]
    if C > LENS_MAX_CAMERAS:
        raise ValueError(f"{name}: at most {LENS_MAX_CAMERAS} cameras a call, got {C}")
    d = lens_coeffs(dist)
    if d.ndim > 2 or (d.ndim == 2 and d.shape[0] not in (1, C)):
        raise ValueError(f"{name}: dist must be [k] or [{C}, k], got {list(d.shape)}")
    d = np.ascontiguousarray(np.broadcast_to(d.reshape(-1, 12), (C, 12)))
    if per_camera:
        if x.dim() < 3 or x.shape[-3] != C:
            raise ValueError(f"{name}: K holds {C} cameras, so points must be [..., {C}, n, {last}], got {list(x.shape)}")
        outer, n = int(np.prod(x.shape[:-3], dtype=np.int64)), int(x.shape[-2])
    else:
        outer, n = 1, int(np.prod(x.shape[:-1], dtype=np.int64))
    return Kh, d, per_camera, outer, C, n


def _hp(a):
    return None if a is None else a.ctypes.data


def distort_points(x: torch.Tensor, K, dist, P=None, normalized: bool = False) -> torch.Tensor:
    """Undistorted points -> where the real lens images them, in one launch: x [..., 2] device tensor, as pixels of P
    (default K) or, normalized=True, as normalised coordinates -> float64 pixels of K.  The exact inverse direction of
    undistort_points with the same arguments.  All-zero coefficients with P equal to K and pixels in: the input object is
    returned unchanged."""
    Kh, d, _pc, outer, C, n = _lens_setup("distort_points", x, K, dist, 2)
    Ph = None if P is None else _lens_matrix("distort_points", "P", P, C)
    if not normalized and not d.any() and (Ph is None or np.array_equal(Ph, Kh)):
        return x
    xi = x.contiguous().to(torch.float64)
    out = torch.empty_like(xi)
    check(lib().skimi_distort_points(ptr(xi), _hp(Kh), _hp(d), _hp(Ph), None, outer, C, n, 1 if normalized else 0, ptr(out),
                                     _lib.current_stream()), "skimi_distort_points")
    return out


def undistort_points(x: torch.Tensor, K, dist, P=None, iters: int = 20, normalized: bool = False) -> UndistortResult:
    """cv2.undistortPoints(x, K, dist, P=P) in one launch: distorted pixels x [..., 2] (device) of K -> UndistortResult(x,
    resid_px), the points as pixels of P (default K) or, normalized=True, as normalised coordinates (cv2's result without
    P).  OpenCV's fixed-point iteration with exactly `iters` rounds (cv2 runs 5; no early exit: bitwise reproducible).
    resid_px is the pixel distance between the input and the re-distorted result: it exposes a point that did not converge
    or lies beyond the model's invertible range.  A NaN keypoint gives NaN in its own row only.  All-zero coefficients
    with P equal to K and pixels out: the input object is returned unchanged, with a zero residual."""
    Kh, d, _pc, outer, C, n = _lens_setup("undistort_points", x, K, dist, 2)
    Ph = None if P is None else _lens_matrix("undistort_points", "P", P, C)
    iters = int(iters)
    if not 0 <= iters <= LENS_MAX_ITERS:
        raise ValueError(f"undistort_points: iters must be in 0..{LENS_MAX_ITERS}, got {iters}")
    if not normalized and not d.any() and (Ph is None or np.array_equal(Ph, Kh)):
        return UndistortResult(x, torch.zeros(x.shape[:-1], dtype=torch.float64, device=x.device))
    xi = x.contiguous().to(torch.float64)
    out = torch.empty_like(xi)
    resid = torch.empty(xi.shape[:-1], dtype=torch.float64, device=xi.device)
    check(lib().skimi_undistort_points(ptr(xi), _hp(Kh), _hp(d), _hp(Ph), None, outer, C, n, iters, 1 if normalized else 0,
                                       ptr(out), ptr(resid), _lib.current_stream()), "skimi_undistort_points")
    return UndistortResult(out, resid)


def undistort_keypoints_steps(keypoints: torch.Tensor, K: torch.Tensor, dist, iters: int = 20) -> UndistortResult:
    """post_triage_single's rule, undistortPoints(x, K, d, P=K), for keypoints [T, V, J, 2] whose K [T, V, 3, 3] is a DEVICE
    tensor with one matrix per step and view (the model's own intrinsics): the kernel reads K from memory, the per-view
    coefficients dist ([k] or [V, k]) travel by value.  One launch; float64 out."""
    if keypoints.dim() != 4 or keypoints.shape[-1] != 2 or tuple(K.shape) != tuple(keypoints.shape[:2]) + (3, 3):
        raise ValueError(f"undistort_keypoints_steps: need keypoints [T, V, J, 2] and K [T, V, 3, 3], got {list(keypoints.shape)}, "
                         f"{list(K.shape)}")
    if not keypoints.is_cuda or K.device != keypoints.device:
        raise _lib.SkimiError("undistort_keypoints_steps needs keypoints and K on one device")
    T, V, J, _ = keypoints.shape
    if V > LENS_MAX_CAMERAS:
        raise ValueError(f"undistort_keypoints_steps: at most {LENS_MAX_CAMERAS} views, got {V}")
    d = lens_coeffs(dist)
    if d.ndim > 2 or (d.ndim == 2 and d.shape[0] not in (1, V)):
        raise ValueError(f"undistort_keypoints_steps: dist must be [k] or [{V}, k], got {list(d.shape)}")
    d = np.ascontiguousarray(np.broadcast_to(d.reshape(-1, 12), (V, 12)))
    xi = keypoints.contiguous().to(torch.float64)
    Kd = K.contiguous().to(torch.float64)
    out = torch.empty_like(xi)
    resid = torch.empty((T, V, J), dtype=torch.float64, device=xi.device)
    check(lib().skimi_undistort_points(ptr(xi), None, _hp(d), None, ptr(Kd), T, V, J, int(iters), 0, ptr(out), ptr(resid),
                                       _lib.current_stream()), "skimi_undistort_points")
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
    Rh, th = _host_f64(R), _host_f64(t)
    if tuple(Rh.shape) != ((C, 3, 3) if per_camera else (3, 3)) or tuple(th.shape) != ((C, 3) if per_camera else (3,)):
        raise ValueError(f"project_points: R / t must match K ({'[C, 3, 3] / [C, 3]' if per_camera else '[3, 3] / [3]'}), got "
                         f"{list(Rh.shape)}, {list(th.shape)}")
    if not (np.isfinite(Rh).all() and np.isfinite(th).all()):
        raise ValueError("project_points: R and t must be finite")
    Xi = X.contiguous().to(torch.float64)
    px = torch.empty(Xi.shape[:-1] + (2,), dtype=torch.float64, device=Xi.device)
    depth = torch.empty(Xi.shape[:-1], dtype=torch.float64, device=Xi.device)
    check(lib().skimi_project_points(ptr(Xi), _hp(Rh), _hp(th), _hp(Kh), _hp(d), outer, C, n, ptr(px), ptr(depth),
                                     _lib.current_stream()), "skimi_project_points")
    return ProjectResult(px, depth)


# ---- bird's-eye view: front_side/front/bev_utils.py, front_side/run.py (csrc/bev.hip; rules: include/skimi.h, DESIGN §2
# "Bird's-eye view"; the reference's names and the clip entry point: bev.py) ---------------------------------------------
HOMOGRAPHY_STAT_FIELDS = ("n_used", "rms_err", "max_err", "det")
TRACK_FIELDS = ("step", "path", "vx", "vy", "speed", "heading")


@dataclass
class HomographyResult:
    """homography_fit's outputs (device tensors; a leading group axis only when the input had one)."""
    H: torch.Tensor          # float64 [.., 3, 3]: post @ Hn, maps src to post's frame; NaN for a failed group
    Hinv: torch.Tensor       # float64 [.., 3, 3]: adj(H) / det(H), what preprocess.warp_perspective takes
    Hn: torch.Tensor         # float64 [.., 3, 3]: the fit itself, before post (the reference's H_m beside H_px = S @ H_m)
    err: torch.Tensor        # float64 [.., n]: transfer error of every used point in post's frame, NaN for an unused one
    stats: torch.Tensor      # float64 [.., 4]: HOMOGRAPHY_STAT_FIELDS (det is that of Hn, before post)
    status: torch.Tensor     # bool [..]: Hn finite and |det Hn| >= 1e-12 (the reference's check_homography)


class BevSkeletonResult(NamedTuple):
    """bev_skeleton's outputs (device tensors)."""
    uv: torch.Tensor             # float64 [T, J, 2]: unrounded plan pixels, NaN for an invalid joint
    px: torch.Tensor             # int32 [T, J, 2]: rounded half to even, 0 for an invalid joint
    valid: torch.Tensor          # bool [T, J]
    center_world: torch.Tensor   # float64 [T, 3]: np.nanmean over the joints per coordinate


class GroundTrackResult(NamedTuple):
    """ground_track's outputs (device tensors, views of `table`)."""
    table: torch.Tensor      # float64 [P, T, 6]: TRACK_FIELDS
    step: torch.Tensor       # [P, T] metres moved since the previous sample (0 at t = 0, NaN next to a gap)
    path: torch.Tensor       # [P, T] the running sum of the finite steps
    velocity: torch.Tensor   # [P, T, 2] metres per second, central differences
    speed: torch.Tensor      # [P, T]
    heading: torch.Tensor    # [P, T] atan2(vx, vy): 0 along +y (down the lane), positive towards +x


def homography_fit(src: torch.Tensor, dst: torch.Tensor, post=None) -> HomographyResult:
    """cv2.findHomography(src, dst, method=0) without its Levenberg-Marquardt polish, for G independent groups in one launch:
    src, dst [n, 2] or [G, n, 2] device tensors, n >= 4 (a correspondence with a non-finite number is skipped); post a host
    [3, 3] composed on the left (H = post @ Hn: the canvas matrix S of bev.make_bev_canvas) -> HomographyResult.  Hartley
    normalisation, the 9 x 9 normal matrix, cyclic Jacobi, the eigenvector of the smallest eigenvalue: for n > 4 the
    algebraic least-squares solution; RANSAC and LMedS are out.  A degenerate group (fewer than 4 usable points, all points
    of a side coincident, |det| < 1e-12) is NaN with status False; the others are not affected.  Nothing is read back."""
    s, d = _f64_dev("homography_fit", src), _f64_dev("homography_fit", dst)
    grouped = s.dim() == 3
    if s.dim() not in (2, 3) or s.shape[-1] != 2 or d.shape != s.shape:
        raise ValueError(f"homography_fit: src and dst must both be [n, 2] or [G, n, 2], got {list(s.shape)}, {list(d.shape)}")
    if not grouped:
        s, d = s[None], d[None]
    G, n = int(s.shape[0]), int(s.shape[1])
    if n < 4 or G < 1:
        raise ValueError(f"homography_fit: at least 4 correspondences and one group, got n = {n}, G = {G}")
    ph = None
    if post is not None:
        ph = _host_f64(post)
        if ph.shape != (3, 3) or not np.isfinite(ph).all():
            raise ValueError(f"homography_fit: post must be a finite [3, 3], got shape {list(ph.shape)}")
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=s.device)   # noqa: E731
    H, Hinv, Hn, err, stats = f64(G, 3, 3), f64(G, 3, 3), f64(G, 3, 3), f64(G, n), f64(G, 4)
    status = torch.empty((G,), dtype=torch.int32, device=s.device)
    check(lib().skimi_homography_fit(ptr(s), ptr(d), _hp(ph), G, n, ptr(H), ptr(Hinv), ptr(Hn), ptr(err), ptr(stats), ptr(status),
                                     _lib.current_stream()), "skimi_homography_fit")
    res = (H, Hinv, Hn, err, stats, status.bool())
    return HomographyResult(*(res if grouped else (a[0] for a in res)))


def homography_points(x: torch.Tensor, H: torch.Tensor, eps: float = 1e-8) -> torch.Tensor:
    """bev_utils.image_points_to_bev in one launch: x [..., n, 2] and H device tensors -> float64 [..., n, 2].  H [3, 3] serves
    every point; H [..., 3, 3] with x's leading axes gives every group of n points its own (a matrix per frame).  Where the
    reference raises (|w| < eps) and where the point or w is not finite, the point is NaN in both coordinates and no other."""
    if not isinstance(H, torch.Tensor) or not H.is_cuda:
        raise _lib.SkimiError("homography_points needs the matrices on the device")
    xi, Hd = _f64_dev("homography_points", x), _f64_dev("homography_points", H, x.device if isinstance(x, torch.Tensor) else None)
    if xi.dim() < 1 or xi.shape[-1] != 2:
        raise ValueError(f"homography_points: points must be [..., 2], got {list(xi.shape)}")
    if tuple(Hd.shape) == (3, 3):
        shared, G, n = 1, 1, xi.numel() // 2
    else:
        if xi.dim() < 2 or Hd.shape[-2:] != (3, 3) or tuple(Hd.shape[:-2]) != tuple(xi.shape[:-2]):
            raise ValueError(f"homography_points: H must be [3, 3] or match the points' leading axes, got H {list(Hd.shape)} "
                             f"for points {list(xi.shape)}")
        shared, n = 0, int(xi.shape[-2])
        G = xi.numel() // 2 // n if n else 0
    if not float(eps) >= 0.0:
        raise ValueError(f"homography_points: eps must be >= 0, got {eps}")
    out = torch.empty_like(xi)
    check(lib().skimi_homography_points(ptr(xi), ptr(Hd), G, n, shared, float(eps), ptr(out), _lib.current_stream()),
          "skimi_homography_points")
    return out


def bev_skeleton(X: torch.Tensor, center_px: torch.Tensor, metres_per_pixel: float = 0.02, use_axes=(0, 2),
                 rot90_left: bool = False, center_world=None) -> BevSkeletonResult:
    """front_side/run.py: project_world_to_bev_centered with merge's centre, for a whole clip in one launch: X [T, J, 3] (or
    [J, 3]) world joints, center_px [T, 2] (or [2]) the plan pixel the skeleton is centred on (merge: the last box's foot
    point), device tensors -> BevSkeletonResult.  The centre in the world is np.nanmean over the joints per coordinate; a
    joint with a non-finite coordinate (the reference's None), or a step whose centre is not finite, is invalid: NaN in
    uv, 0 in px.  px rounds half to even, as Python's round does in the reference.  center_world [T, 3] (device): a centre of
    the caller's in place of the mean."""
    Xd = _f64_dev("bev_skeleton", X)
    single = Xd.dim() == 2
    if single:
        Xd = Xd[None]
    if Xd.dim() != 3 or Xd.shape[2] != 3 or Xd.shape[1] < 1:
        raise ValueError(f"bev_skeleton: need X [T, J, 3], got {list(X.shape)}")
    T, J = int(Xd.shape[0]), int(Xd.shape[1])
    c = _f64_dev("bev_skeleton", center_px, Xd.device)
    if tuple(c.shape) not in ((T, 2), (2,) if single else (T, 2)):
        raise ValueError(f"bev_skeleton: center_px must be [{T}, 2], got {list(c.shape)}")
    ax0, ax1 = (int(a) for a in use_axes)
    if not (0 <= ax0 <= 2 and 0 <= ax1 <= 2):
        raise ValueError(f"bev_skeleton: use_axes must be two of 0, 1, 2, got {use_axes}")
    if not float(metres_per_pixel) > 0.0:
        raise ValueError(f"bev_skeleton: metres_per_pixel must be positive, got {metres_per_pixel}")
    dev = Xd.device
    cin = None
    if center_world is not None:
        cin = _f64_dev("bev_skeleton", center_world, dev)
        if tuple(cin.shape) not in ((T, 3), (3,) if single else (T, 3)):
            raise ValueError(f"bev_skeleton: center_world must be [{T}, 3], got {list(cin.shape)}")
    uv = torch.empty((T, J, 2), dtype=torch.float64, device=dev)
    px = torch.empty((T, J, 2), dtype=torch.int32, device=dev)
    valid = torch.empty((T, J), dtype=torch.uint8, device=dev)
    cw = torch.empty((T, 3), dtype=torch.float64, device=dev)
    check(lib().skimi_bev_skeleton(ptr(Xd), ptr(c), ptr(cin), T, J, float(metres_per_pixel), ax0, ax1, int(bool(rot90_left)), ptr(uv), ptr(px),
                                   ptr(valid), ptr(cw), _lib.current_stream()), "skimi_bev_skeleton")
    res = (uv, px, valid.bool(), cw)
    return BevSkeletonResult(*((a[0] for a in res) if single else res))


def ground_track(p: torch.Tensor, fps: float = 30.0) -> GroundTrackResult:
    """The metric ground track of P people in one launch: p [P, T, 2] (or [T, 2]) positions on the ground plane in metres
    (bev.process_front_clip's foot_m), NaN = no detection -> GroundTrackResult: the step and the path length, the velocity
    by central differences (one-sided at the two ends), the speed and the heading atan2(vx, vy).  A value next to a gap is
    NaN; the path sums the finite steps only.  NOTHING IS SMOOTHED INSIDE: a box's foot point jitters by pixels, which the
    differences amplify, so smooth the track first with smooth_savgol or smooth_ema (as [T, P, 3] with a zero third
    coordinate) and pass the result."""
    pd = _f64_dev("ground_track", p)
    single = pd.dim() == 2
    if single:
        pd = pd[None]
    if pd.dim() != 3 or pd.shape[2] != 2:
        raise ValueError(f"ground_track: need p [P, T, 2], got {list(p.shape)}")
    if not float(fps) > 0.0:
        raise ValueError(f"ground_track: fps must be positive, got {fps}")
    P, T = int(pd.shape[0]), int(pd.shape[1])
    out = torch.empty((P, T, 6), dtype=torch.float64, device=pd.device)
    check(lib().skimi_ground_track(ptr(pd), P, T, float(fps), ptr(out), _lib.current_stream()), "skimi_ground_track")
    if single:
        out = out[0]
    return GroundTrackResult(out, out[..., 0], out[..., 1], out[..., 2:4], out[..., 4], out[..., 5])


# ---- host helpers of the wrapper (small arrays, NumPy as in the reference) -----------------
# ---- camera calibration from chessboard corners (camera_calibration/main.py; DESIGN §2 "Calibration") ----
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
    for a in (obj, img, use, K0, dist0):
        if a is not None and (not isinstance(a, torch.Tensor) or not a.is_cuda):
            raise _lib.SkimiError("calibrate_camera needs device tensors")
    if obj.dim() != 2 or obj.shape[1] != 2 or img.dim() != 3 or img.shape[1:] != (obj.shape[0], 2):
        raise ValueError(f"calibrate_camera: need obj [n, 2] and img [V, n, 2], got {list(obj.shape)}, {list(img.shape)}")
    mask = calib_free_mask(free, rational_model, zero_tangent)
    width, height = (int(x) for x in image_size)
    dev = obj.device
    V, n = int(img.shape[0]), int(img.shape[1])
    if K0 is not None and K0.dim() == 2:
        K0 = K0[None]
    if dist0 is not None and dist0.dim() == 1:
        dist0 = dist0[None]
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
    obj, img = obj.to(dev, torch.float64).contiguous(), img.to(dev, torch.float64).contiguous()
    if use is not None:
        use = (use != 0).to(dev, torch.uint8).contiguous()
    if K0 is not None:
        K0 = K0.to(dev, torch.float64).contiguous()
    if dist0 is not None:
        d = torch.zeros((G, 12), dtype=torch.float64, device=dev)
        d[:, :dist0.shape[1]] = dist0
        dist0 = d
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)   # noqa: E731
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)     # noqa: E731
    K, dist, R, t, rvec, err, stats = f64(G, 3, 3), f64(G, 12), f64(G, V, 3, 3), f64(G, V, 3), f64(G, V, 3), f64(G, V, n), f64(G, V, 3)
    rms, c0, c, std, ne, nv, nc, ok = f64(G), f64(G), f64(G), f64(G, 12), i32(G), i32(G), i32(G), i32(G)
    nws = int(lib().skimi_calibrate_workspace_bytes(G, V, n))
    ws = torch.empty(max(nws, 8), dtype=torch.uint8, device=dev)
    check(lib().skimi_calibrate_camera(ptr(obj), ptr(img), ptr(use), ptr(K0), ptr(dist0), G, V, n, width, height, mask, int(max_evals),
                                       ptr(K), ptr(dist), ptr(R), ptr(t), ptr(rvec), ptr(err), ptr(stats), ptr(rms), ptr(c0), ptr(c),
                                       ptr(std), ptr(ne), ptr(nv), ptr(nc), ptr(ok), ptr(ws), nws, _lib.current_stream()),
          "skimi_calibrate_camera")
    return CalibrationResult(K, dist, R, t, rvec, err, stats[..., 0], stats[..., 1], stats[..., 2], rms, c0, c, std, ne, nv, nc,
                             ok.bool())


def extrinsic_to_RT(extrinsic):
    """vggt/vggt/infer.py:107-126: E (T,3,4)|(T,4,4)|(3,4)|(4,4) -> R (T,3,3), t (T,3), C = -R^T t"""
    E = np.asarray(extrinsic)
    if E.ndim == 2:
        E = E[None, ...]
    if E.shape[-2:] == (4, 4):
        E = E[:, :3, :]
    R = E[:, :3, :3]
    t = E[:, :3, 3]
    C = -np.einsum("tij,tj->ti", R.transpose(0, 2, 1), t)
    return R, t, C


def scale_intrinsics(K: np.ndarray, orig_size, new_size) -> np.ndarray:
    """vggt/vggt/infer.py:128-155: rescale K from `orig_size` (H, W) pixels to `new_size`."""
    H0, W0 = orig_size
    H1, W1 = new_size
    sx, sy = W1 / W0, H1 / H0
    K_new = K.copy().astype(float)
    K_new[0, 0] *= sx
    K_new[1, 1] *= sy
    K_new[0, 2] *= sx
    K_new[1, 2] *= sy
    return K_new
