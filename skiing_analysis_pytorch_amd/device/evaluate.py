"""Pose evaluation of clips: the MPJPE protocols and the ground-truth-free quality figures (csrc/evaluate.hip; C-ABI:
skimi_eval_workspace_bytes, skimi_pose_errors, skimi_clip_quality): VideoPose3D/common/loss.py, fuse/fuse_eval.py,
metrics/unity_data_compare.py, metrics/true_data_compare.py; the reference's names are the package's evaluate.py; rules:
include/skimi.h, DESIGN §2 "Evaluation".
"""
from __future__ import annotations

from typing import NamedTuple

import torch

from .._args import clips, f64, i32, index_list, lengths as clip_lengths, workspace
from .._lib import check, current_stream, lib, ptr

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


def pose_errors(pred: torch.Tensor, target: torch.Tensor, lengths=None, zero_root=None, aligned: bool = False) -> PoseErrorsResult:
    """The MPJPE protocols of VideoPose3D/common/loss.py (mpjpe, p_mpjpe, n_mpjpe, mean_velocity_error) and the per-joint
    tables of metrics/unity_data_compare.py for a batch of (prediction, target) clips in three launches: pred, target
    [B, T, J, 3] (a [T, J, 3] input is one clip) device tensors, J <= 128; lengths None or [B] integers, 0 <= length <= T (the
    frames beyond a clip's length are never read); zero_root None or a joint index: that joint of the target counts as (0, 0,
    0), evaluate()'s `inputs_3d[:, :, 0] = 0`, and the input is not written -> PoseErrorsResult.  aligned=True also returns
    the aligned prediction with its rotation, scale and translation.  Nothing is read back."""
    P, G = clips("pose_errors", pred), clips("pose_errors", target)
    if P.shape != G.shape:
        raise ValueError(f"pose_errors: pred {list(P.shape)} and target {list(G.shape)} differ")
    if G.device != P.device:
        raise ValueError("pose_errors: pred and target live on different devices")
    B, T, J = (int(s) for s in P.shape[:3])
    dev = P.device
    len_t = clip_lengths("pose_errors", lengths, B, dev)
    err, p_err, vel = f64(dev, B, T, J), f64(dev, B, T, J), f64(dev, B, T, J)
    mf, nf, pf, nv, st = f64(dev, B, T), f64(dev, B, T), f64(dev, B, T), i32(dev, B, T), i32(dev, B, T)
    al, pR, ps, pt = (f64(dev, B, T, J, 3), f64(dev, B, T, 3, 3), f64(dev, B, T), f64(dev, B, T, 3)) if aligned else (None,) * 4
    metrics, counts, jstats, jn = f64(dev, B, 4), i32(dev, B, 3), f64(dev, B, 2, J, 3), i32(dev, B, 2, J)
    check(lib().skimi_pose_errors(ptr(P), ptr(G), ptr(len_t), B, T, J, -1 if zero_root is None else int(zero_root), ptr(err), ptr(p_err),
                                  ptr(vel), ptr(mf), ptr(nf), ptr(pf), ptr(nv), ptr(st), ptr(al), ptr(pR), ptr(ps), ptr(pt), ptr(metrics),
                                  ptr(counts), ptr(jstats), ptr(jn), current_stream()), "skimi_pose_errors")
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
    X = clips("clip_quality", X)
    if placement not in ("auto", "workspace"):
        raise ValueError("placement must be 'auto' or 'workspace'")
    B, T, J = (int(s) for s in X.shape[:3])
    dev = X.device
    len_t = clip_lengths("clip_quality", lengths, B, dev)
    (e_c, E), (l_c, EL), (r_c, ER) = (index_list("clip_quality", w, v, EVAL_MAX_EDGES) for w, v in
                                      (("edges", edges), ("left_edges", left_edges), ("right_edges", right_edges)))
    p_c, NP = index_list("clip_quality", "lr_pairs", lr_pairs, EVAL_MAX_PAIRS)
    scalars, cv_edge, bone_len = f64(dev, B, 8), f64(dev, B, E), f64(dev, B, T, E)
    ws, ws_bytes = None, 0
    if placement == "workspace" or T * J > EVAL_LDS_ELEMS:
        ws_bytes = int(lib().skimi_eval_workspace_bytes(B, T, J))
        ws = workspace(dev, ws_bytes, at_least=8, as_f64=True) if B and T else None
    check(lib().skimi_clip_quality(ptr(X), ptr(len_t), B, T, J, e_c, E, l_c, EL, r_c, ER, p_c, NP, ptr(ws), ws_bytes, ptr(scalars),
                                   ptr(cv_edge), ptr(bone_len), current_stream()), "skimi_clip_quality")
    return ClipQualityResult(*(scalars[:, k] for k in range(8)), cv_edge, bone_len, scalars)
