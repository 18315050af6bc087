"""The skiing analysis proper, angle/main.py of the reference: joint angles, body tilt, torso-knee angle, knee difference and
elbow distances per frame, their frame-to-frame changes, the skier's facing heading, the split of a run into turns and the
per-turn statistics -- all from ONE geometry.kinematics call on the device (csrc/kinematics.hip; rules: include/skimi.h,
DESIGN §2 "Kinematics"), where the reference loops over the frames on the host once per series.  The host part is what is
left: reading the results back and writing the reference's CSV files under its directory names, with its headers and row
order.  No PNG is written: not the series plots, not the skeleton pictures, not the elbow-position picture.

The tables below restate the reference's as data.  A layout names the joint of each role (geometry.KIN_ROLES order, -1 for
absent) in a clip's joint axis: MHR70_15 is the reference's own 15-joint order, H36M_17 this build's fused VideoPose3D joints
with the thorax as the neck.  COCO_17 stands for the COCO-17 joints of the VGGT clip path: they have no neck, so analyze and
process_person_pair convert them on the device (geometry.convert_skeleton, "coco_to_h36m") and run the H36M_17 layout."""
from __future__ import annotations

import csv
from pathlib import Path
from typing import Dict, List, NamedTuple

import numpy as np
import torch

from . import geometry

UNITY_MHR70_MAPPING = {1: "Bone_Eye_L", 2: "Bone_Eye_R", 5: "Upperarm_L", 6: "Upperarm_R", 7: "lowerarm_l", 8: "lowerarm_r",
                       9: "Thigh_L", 10: "Thigh_R", 11: "calf_l", 12: "calf_r", 13: "Foot_L", 14: "Foot_R", 41: "Hand_R",
                       62: "Hand_L", 69: "neck_01"}
TARGET_IDS = list(UNITY_MHR70_MAPPING)
ID_TO_INDEX = {jid: idx for idx, jid in enumerate(TARGET_IDS)}
ANGLE_DEFS = {"knee_l": (9, 11, 13), "knee_r": (10, 12, 14), "elbow_l": (5, 7, 62), "elbow_r": (6, 8, 41),
              "shoulder_l": (69, 5, 7), "shoulder_r": (69, 6, 8), "hip_l": (69, 9, 11), "hip_r": (69, 10, 12)}
ELBOW_IDS = {"elbow_l": 7, "elbow_r": 8}
# the MHR-70 id of each role, geometry.KIN_ROLES order
ROLE_IDS = (5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 62, 41, 69)

MHR70_15 = tuple(ID_TO_INDEX[i] for i in ROLE_IDS)
H36M_17 = (11, 14, 12, 15, 4, 1, 5, 2, 6, 3, 13, 16, 8)     # Human3.6M: hips 4 / 1, knees 5 / 2, feet 6 / 3, thorax 8, arms 11-13 / 14-16
COCO_17 = ("coco17",)                                       # not a role table: _role_layout converts to H36M-17 first
assert MHR70_15 == geometry.KIN_LAYOUT_MHR70_15

SERIES = geometry.KIN_SERIES
UP_Y_DOWN = (0.0, -1.0, 0.0)
# the per-series files of a report and the series each holds, in the reference's order
SERIES_FILES = {
    "angles_joint.csv": SERIES[0:8],
    "angles_knee.csv": SERIES[0:2],
    "angles_torso_knee.csv": SERIES[8:9],
    "angles_knee_diff.csv": SERIES[9:10],
    "distance_elbow_midline.csv": SERIES[10:12],
    "angles_body_y_down.csv": SERIES[12:14],
    "angles_change_fullframe.csv": SERIES[14:],
}
TURN_FIELDS = ("turn_id", "start_frame", "end_frame", "num_frames", "heading_change_deg", "direction")


class Analysis(NamedTuple):
    """One clip's analysis on the host."""
    series: Dict[str, np.ndarray]    # the 42 series [T] in SERIES order
    heading: np.ndarray              # [T] degrees
    turns: List[Dict[str, float]]    # the reference's turn dicts (TURN_FIELDS, floats, turn_id from 1)
    stats: np.ndarray                # [turns, 42, 4]: mean, population std, min, max over each turn's finite samples
    counts: np.ndarray               # [turns, 42]


def analysis_from(result, clip: int = 0, length: int | None = None) -> Analysis:
    """Clip `clip` of a geometry.KinematicsResult (read back here) or of a mapping with the same field names holding host
    arrays -> Analysis, cut to the clip's `length` frames."""
    get = (lambda k: result[k]) if isinstance(result, dict) else (lambda k: getattr(result, k))      # noqa: E731
    host = lambda k: (get(k)[clip].cpu().numpy() if isinstance(get(k), torch.Tensor) else np.asarray(get(k)[clip]))   # noqa: E731
    every = np.concatenate([host("series"), host("changes")], axis=0)
    T = every.shape[1] if length is None else int(length)
    n = int(host("n_turns"))
    frames, dh, direction = host("turn_frames"), host("turn_heading_change"), host("turn_direction")
    turns = [{"turn_id": float(t + 1), "start_frame": float(frames[t, 0]), "end_frame": float(frames[t, 1]),
              "num_frames": float(frames[t, 1] - frames[t, 0] + 1), "heading_change_deg": float(dh[t]),
              "direction": 1.0 if direction[t] > 0 else -1.0} for t in range(n)]
    return Analysis({name: every[k, :T] for k, name in enumerate(SERIES)}, host("heading")[:T], turns, host("turn_stats")[:n],
                    host("turn_counts")[:n])


def _role_layout(kpts: torch.Tensor, layout):
    """(device joints (..., J, 3), layout) as geometry.kinematics takes them: COCO_17 joints are converted to H36M-17 frame by
    frame (geometry.convert_skeleton, "coco_to_h36m") and get the H36M_17 roles; any other layout passes through"""
    if tuple(layout) != COCO_17:
        return kpts, layout
    if kpts.shape[-2] != 17:
        raise ValueError(f"layout COCO_17 needs 17 joints, got {kpts.shape[-2]}")
    return geometry.convert_skeleton(kpts.reshape(-1, 17, 3), "coco_to_h36m").reshape(kpts.shape), H36M_17


def analyze(kpts, up_axis=UP_Y_DOWN, layout=MHR70_15, **kw) -> Analysis:
    """kpts (T, J, 3), a host array or a device tensor -> Analysis, from one device call (two for layout=COCO_17: the
    conversion to H36M-17 comes first)."""
    if not isinstance(kpts, torch.Tensor):
        kpts = torch.from_numpy(np.ascontiguousarray(np.asarray(kpts, dtype=np.float64))).to(torch.device("cuda", torch.cuda.current_device()))
    if kpts.dim() != 3 or kpts.shape[2] != 3:
        raise ValueError("kpts must be (T,J,3)")
    kpts, layout = _role_layout(kpts, layout)
    return analysis_from(geometry.kinematics(kpts, layout=layout, up_axis=up_axis, **kw))


def compute_all_series(kpts, up_axis=UP_Y_DOWN, layout=MHR70_15):
    """angle/main.py's _compute_all_series: -> (joint_angles, body_angles, torso_knee, knee_diff, elbow_dist, heading_deg,
    turns): five dicts of NumPy series, the heading and the list of turn dicts."""
    a = analyze(kpts, up_axis, layout)
    pick = lambda names: {n: a.series[n] for n in names}      # noqa: E731
    return (pick(SERIES[0:8]), pick(SERIES[12:14]), pick(SERIES[8:9]), pick(SERIES[9:10]), pick(SERIES[10:12]), a.heading, a.turns)


# ---- the reference's files ---------------------------------------------------------------------------------------------
def _num(v):
    return float(v)      # csv writes repr(float): the shortest text that reads back to the same bits, "nan" for NaN


def save_angles_csv(out_path: Path, angles: Dict[str, np.ndarray]) -> None:
    names = list(angles)
    T = len(next(iter(angles.values()))) if angles else 0
    out_path = Path(out_path)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    with out_path.open("w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["frame"] + names)
        for t in range(T):
            w.writerow([t] + [_num(angles[n][t]) for n in names])


def save_fullframe_reports(output_dir: Path, a: Analysis, files=tuple(SERIES_FILES), start: int = 0, end: int | None = None) -> None:
    """the per-series files of SERIES_FILES for the frames start .. end (inclusive), numbered from 0"""
    stop = None if end is None else end + 1
    for fname in files:
        save_angles_csv(Path(output_dir) / fname, {n: a.series[n][start:stop] for n in SERIES_FILES[fname]})


def _stat_row(a: Analysis, t: int, k: int):
    return [_num(v) for v in a.stats[t, k]] if a.counts[t, k] > 0 else ["nan"] * 4


def save_turn_reports(output_dir: Path, a: Analysis) -> None:
    """turn_summary.csv, turn_metrics.csv, turn_heading.csv and turn_details/ (save_turn_reports + save_turn_detail_files)"""
    output_dir = Path(output_dir)
    output_dir.mkdir(parents=True, exist_ok=True)
    with (output_dir / "turn_summary.csv").open("w", newline="") as f:
        w = csv.writer(f)
        w.writerow(list(TURN_FIELDS))
        for turn in a.turns:
            w.writerow([int(turn["turn_id"]), int(turn["start_frame"]), int(turn["end_frame"]), int(turn["num_frames"]),
                        turn["heading_change_deg"], "left" if turn["direction"] > 0 else "right"])
    with (output_dir / "turn_metrics.csv").open("w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["turn_id", "metric", "mean", "std", "min", "max"])
        for t, turn in enumerate(a.turns):
            for k, name in enumerate(SERIES):
                w.writerow([int(turn["turn_id"]), name] + _stat_row(a, t, k))
    boundaries = {int(turn[k]) for turn in a.turns for k in ("start_frame", "end_frame")}
    with (output_dir / "turn_heading.csv").open("w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["frame", "heading_deg", "turn_boundary"])
        for i, h in enumerate(a.heading):
            w.writerow([i, _num(h), 1 if i in boundaries else 0])
    root = output_dir / "turn_details"
    root.mkdir(parents=True, exist_ok=True)
    for t, turn in enumerate(a.turns):
        tid, s, e = int(turn["turn_id"]), int(turn["start_frame"]), int(turn["end_frame"])
        d = root / f"turn_{tid}_{s}_{e}"
        d.mkdir(parents=True, exist_ok=True)
        with (d / "series.csv").open("w", newline="") as f:
            w = csv.writer(f)
            w.writerow(["local_frame", "global_frame", "heading_deg"] + list(SERIES))
            for g in range(s, e + 1):
                w.writerow([g - s, g, _num(a.heading[g])] + [_num(a.series[n][g]) for n in SERIES])
        with (d / "summary.csv").open("w", newline="") as f:
            w = csv.writer(f)
            w.writerow(["turn_id", "start_frame", "end_frame", "num_frames", "metric", "mean", "std", "min", "max"])
            for k, name in enumerate(SERIES):
                w.writerow([tid, s, e, e - s + 1, name] + _stat_row(a, t, k))
        save_fullframe_reports(d, a, start=s, end=e)


def save_turn_comparison_report(out_csv: Path, before: Analysis, after: Analysis) -> None:
    """turn_compare_fused_vs_smoothed.csv: the turns paired by order, the per-turn means of every series and their difference"""
    out_csv = Path(out_csv)
    out_csv.parent.mkdir(parents=True, exist_ok=True)
    metrics = sorted(SERIES)
    mean = lambda a, t, k: _num(a.stats[t, k, 0]) if a.counts[t, k] > 0 else float("nan")      # noqa: E731
    with out_csv.open("w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["turn_pair_index", "before_turn_id", "after_turn_id", "metric", "before_mean", "after_mean",
                    "delta_after_minus_before"])
        for i in range(min(len(before.turns), len(after.turns))):
            for m in metrics:
                k = SERIES.index(m)
                mb, ma = mean(before, i, k), mean(after, i, k)
                w.writerow([i + 1, int(before.turns[i]["turn_id"]), int(after.turns[i]["turn_id"]), m, mb, ma, ma - mb])


def write_person(a: Analysis, output_dir: Path) -> None:
    """process_person's files for an analysis at hand: non_turn_evaluation/ and turn_evaluation/ under output_dir"""
    output_dir = Path(output_dir)
    save_fullframe_reports(output_dir / "non_turn_evaluation", a)
    save_turn_reports(output_dir / "turn_evaluation", a)


def write_person_pair(before: Analysis, after: Analysis, output_dir: Path) -> None:
    output_dir = Path(output_dir)
    for sub, a in (("before_smoothed", before), ("after_fused", after)):
        save_fullframe_reports(output_dir / sub / "non_turn_evaluation", a, files=("angles_change_fullframe.csv",))
        save_turn_reports(output_dir / sub / "turn_evaluation", a)
    save_turn_comparison_report(output_dir / "turn_compare_fused_vs_smoothed.csv", before, after)


def process_person(input_path: Path, output_dir: Path, layout=MHR70_15, up_axis=UP_Y_DOWN) -> Analysis:
    """angle/main.py's process_person on a (T, J, 3) .npy clip, without its pictures."""
    a = analyze(np.load(input_path), up_axis, layout)
    write_person(a, output_dir)
    return a


def process_person_pair(smoothed_path: Path, fused_path: Path, output_dir: Path, layout=MHR70_15, up_axis=UP_Y_DOWN):
    """angle/main.py's process_person_pair: both clips in ONE device call (a batch of two with their own lengths), the turn
    reports of each and the comparison of their turns by order."""
    clips = [np.asarray(np.load(p), dtype=np.float64) for p in (smoothed_path, fused_path)]
    for c in clips:
        if c.ndim != 3 or c.shape[2] != 3:
            raise ValueError("kpts must be (T,J,3)")
    if clips[0].shape[1] != clips[1].shape[1]:
        raise ValueError(f"process_person_pair: {clips[0].shape[1]} and {clips[1].shape[1]} joints")
    lengths = [c.shape[0] for c in clips]
    X = np.full((2, max(lengths), clips[0].shape[1], 3), np.nan)
    for b, c in enumerate(clips):
        X[b, :lengths[b]] = c
    dev = torch.device("cuda", torch.cuda.current_device())
    Xd, layout = _role_layout(torch.from_numpy(X).to(dev), layout)
    res = geometry.kinematics(Xd, lengths=lengths, layout=layout, up_axis=up_axis)
    before, after = (analysis_from(res, b, lengths[b]) for b in range(2))
    write_person_pair(before, after, output_dir)
    return before, after
