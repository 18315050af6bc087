"""The public surface of the device-side geometry post-processing: every wrapper of the modules under device/ (one per
kernel file of csrc/; the module map is in INTEGRATION.md) under the name the callers use, geometry.<name>, plus the two
small host helpers of the reference's VGGT wrapper (vggt/vggt/infer.py:107-155).

Every name is imported explicitly, so a name that goes missing is an import error here and not an AttributeError later.
"""
from __future__ import annotations

import numpy as np

# every import below is a re-export (flake8: F401 does not apply in this file); _lib, lib and _undistorted_f32 are kept
# for the callers and tests that reach the library or the dist=None identity rule through geometry
from . import _lib
from ._lib import lib
from .device.triangulation import (pose_encoding_to_extri_intri, unproject_depth_map_to_point_map, triangulate_joints,
                                   TriageResult, VIEW_STAT_FIELDS, triage_launch, triangulate_triage, RobustResult,
                                   ROBUST_MAX_VIEWS, ROBUST_MAX_JOINTS, ROBUST_MAX_REFINE_ITERS, robust_launch,
                                   triangulate_robust)
from .device.person import (PersonOrigin, person_stats, person_origin, recenter_cameras)
from .device.scene import (SCENE_MAX_PIXELS, SceneCloud, scene_launch, scene_point_cloud)
from .device.icp import (estimate_normals, icp_correspondences, ICPResult, icp_point_to_plane)
from .device.ba import (BA_MODES, BA_WEIGHT_KEYS, BA_PLACEMENTS, BAResult, ba_weights, bundle_adjust)
from .device.resect import (RESECT_LOSSES, ResectResult, relative_pose, resect_cameras)
from .device.refine import (RefineResult, refine_cameras_points)
from .device.essential import (EssentialResult, essential_ransac, five_point)
from .device.fuse import (FUSE_MAX_JOINTS, FUSE_SCALE_MODES, SAVGOL_MAX_WIN, FuseH36MResult, FUSE_DIAG_FIELDS,
                          FuseViewsResult, EmaResult, SavgolResult, fuse_h36m, fuse_views, smooth_ema, smooth_savgol,
                          FuseGroupResult, JointQualityResult, fuse_group, joint_quality)
from .device.skeleton import (SKELETON_DIRECTIONS, convert_skeleton)
from .device.kinematics import (KIN_ROLES, KIN_BASE_SERIES, KIN_SERIES, KIN_STAT_FIELDS, KIN_LAYOUT_MHR70_15, KIN_LDS_FRAMES,
                                KinematicsResult, kin_max_turns, kinematics)
from .device.evaluate import (EVAL_MAX_JOINTS, EVAL_MAX_EDGES, EVAL_MAX_PAIRS, EVAL_LDS_ELEMS, JOINT_STAT_FIELDS, H36M_EDGES,
                              H36M_LR_PAIRS, H36M_LEFT_BONES, H36M_RIGHT_BONES, MHR70_15_EDGES, MHR70_15_LEFT_BONES,
                              MHR70_15_RIGHT_BONES, MHR70_15_LR_PAIRS, PoseErrorsResult, ClipQualityResult, pose_errors,
                              clip_quality)
from .device.lens import (LENS_MAX_CAMERAS, LENS_MAX_ITERS, LENS_COEFF_COUNTS, UndistortResult, ProjectResult, lens_coeffs,
                          distort_points, undistort_points, undistort_keypoints_steps, project_points)
from .device.bev import (HOMOGRAPHY_STAT_FIELDS, TRACK_FIELDS, HomographyResult, BevSkeletonResult, GroundTrackResult,
                         homography_fit, homography_points, bev_skeleton, ground_track)
from .device.calibrate import (CALIB_PARAMS, CalibrationResult, calib_free_mask, calibrate_camera)
from .device.chessboard import (CHESS_MAX_NMS, SUBPIX_MAX_WIN, SUBPIX_MAX_ITERS, ChessCandidates, SubpixResult,
                                chessboard_candidates, corner_subpix)
from .device.features import (ORB_MAX_LEVELS, ORB_MAX_FEATURES, ORB_BORDER, OrbFeatures, HammingMatches, orb_pattern,
                              orb_features, match_hamming)
from .device.sift import (SIFT_MAX_OCTAVES, SIFT_MAX_FEATURES, SIFT_MAX_CANDIDATES, SIFT_BORDER, SiftFeatures, L2Matches, sift_taps,
                          sift_octaves, sift_features, match_l2)
from .device.draw import (DRAW_MAX_SHAPES, DRAW_NONE, DRAW_DISC, DRAW_RING, DRAW_CAPSULE, DRAW_GLYPH, GLYPH_ADVANCE, GLYPH_HEIGHT,
                          font_5x7, draw_shapes, pack_colour, disc_shapes, segment_shapes, polyline_shapes, glyph_shapes,
                          string_codes, text_shapes, number_shapes, cat_shapes)
from .device.scene_view import (SCENE_MAX_PRIMS, SCENE_MAX_POINT_SIZE, SCENE_NONE, SCENE_DISC, SCENE_CAPSULE, SCENE_W_ONE,
                                SCENE_WORKSPACE_CAP, CAMERA_AXIS_COLOURS, CAMERA_PRIMS_PER_CAMERA, SceneView, render_scene, host_const,
                                look_at_view, orbit_view, views_from_cameras, view_project, clip_near, disc3d_prims,
                                segment3d_prims, skeleton_prims, camera_centres, camera_prims, grid_prims, cat_prims)
from .device.masks import (MASK_MAX_SIDE, EDT_NONE, NMS_MAX, STATS_FIELDS, ComponentsResult, EdtResult, MaskBoxes, MaskIoU,
                           mask_components, distance_transform, mask_inner_point, pack_masks, mask_boxes, mask_iou, nms_greedy)
from .device.assign import (ASSIGN_MAX, LINK_MAX, Assignment, LinkedBoxes, linear_assignment, link_boxes)
from .device.lens import _undistorted_f32

# ---- host helpers of the wrapper (small arrays, NumPy as in the reference) -----------------
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
