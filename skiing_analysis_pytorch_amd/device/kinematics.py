"""Kinematic analysis of clips: angles, heading, turns (csrc/kinematics.hip; C-ABI: skimi_kin_workspace_bytes,
skimi_kinematics): angle/main.py; the entry points under the reference's names are the package's angle.py; rules:
include/skimi.h, DESIGN §2 "Kinematics".
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple

import numpy as np
import torch

from .._args import clips, f64, i32, lengths as clip_lengths, u8, workspace
from .._lib import check, current_stream, lib, ptr

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
    X = clips("kinematics", X)
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
    len_t = clip_lengths("kinematics", lengths, B, dev)
    M, S = kin_max_turns(T, min_turn_frames), len(KIN_SERIES)
    alls, heading, hs, vs, boundary = f64(dev, B, S, T), f64(dev, B, T), f64(dev, B, T), f64(dev, B, T), u8(dev, B, T)
    n_turns, frames, dh, direction = i32(dev, B), i32(dev, B, M, 2), f64(dev, B, M), i32(dev, B, M)
    stats, counts = f64(dev, B, M, S, 4), i32(dev, B, M, S)
    ws, ws_bytes = None, 0
    if placement == "workspace" or T > KIN_LDS_FRAMES:
        ws_bytes = int(lib().skimi_kin_workspace_bytes(B, T))
        ws = workspace(dev, ws_bytes, at_least=8, as_f64=True) if B and T else None
    check(lib().skimi_kinematics(ptr(X), ptr(len_t), B, T, J, lay_c, up_c, int(min_turn_frames), float(min_heading_change_deg),
                                 int(heading_window), int(velocity_window), M, ptr(ws), ws_bytes, ptr(alls), ptr(heading), ptr(hs),
                                 ptr(vs), ptr(boundary), ptr(n_turns), ptr(frames), ptr(dh), ptr(direction), ptr(stats),
                                 ptr(counts), current_stream()), "skimi_kinematics")
    nb = len(KIN_BASE_SERIES)
    return KinematicsResult(alls[:, :nb], alls[:, nb:], heading, hs, vs, boundary.bool(), n_turns, frames, dh, direction, stats,
                            counts, alls)
