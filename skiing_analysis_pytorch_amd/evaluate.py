"""Pose evaluation on the device, under the reference's names.

The reference evaluates on the host, frame by frame: VideoPose3D/common/loss.py (mpjpe, p_mpjpe, n_mpjpe,
mean_velocity_error) and run.py:951-1049 `evaluate()`, VideoPose3D/fuse/fuse_eval.py `eval_fused_pose` (what
VideoPose3D/main.py:92-102 writes to fused_metrics.txt), metrics/unity_data_compare.py `summarize_joint_errors` and the
ground-truth-free part of metrics/true_data_compare.py `evaluate_person`.  Here all of it sits on two library calls,
geometry.pose_errors and geometry.clip_quality (csrc/evaluate.hip; rules: DESIGN §2 "Evaluation"): the clips stay on the
device, and a function reads back at most once, at its end, and only where it returns host values (a dict).

Deliberate differences: everything runs in float64 (the reference's `evaluate()` runs float32); joints with a non-finite
coordinate are left out of a mean where loss.py would return NaN or raise; P-MPJPE and N-MPJPE of a clip are the mean over
its frames of the per-frame value (equal to the reference's pooled mean on a NaN-free clip, up to rounding).
"""
from __future__ import annotations

import math
from pathlib import Path

import torch

from . import geometry
from ._args import upload_f64

FUSED_METRICS_HEADER = "Fused Pose Evaluation Metrics:"       # VideoPose3D/main.py:100


def _dev(a, like=None):
    """a device float64 tensor of a host array or tensor (a device tensor stays where it is)"""
    if isinstance(a, torch.Tensor) and a.is_cuda:
        return a.to(torch.float64)
    return upload_f64(a, like.device if like is not None else torch.device("cuda", torch.cuda.current_device()))


def _frames(name, a, like=None):
    """(..., J, 3) -> [N, J, 3]: loss.py's means run over every leading axis"""
    a = _dev(a, like)
    if a.dim() < 2 or a.shape[-1] != 3:
        raise ValueError(f"{name}: need (..., J, 3), got {list(a.shape)}")
    return a.reshape(-1, a.shape[-2], 3)


def _pair(name, predicted, target):
    p = _frames(name, predicted)
    g = _frames(name, target, p)
    if p.shape != g.shape:
        raise ValueError(f"{name}: predicted {list(p.shape)} and target {list(g.shape)} differ")
    return p, g


def mpjpe(predicted, target) -> torch.Tensor:
    """loss.py:11-17, Protocol #1: the mean joint distance over (..., J, 3) -> 0-dim device tensor"""
    return geometry.pose_errors(*_pair("mpjpe", predicted, target)).mpjpe[0]


def p_mpjpe(predicted, target) -> torch.Tensor:
    """loss.py:27-66, Protocol #2: the mean joint distance after each frame's similarity alignment -> 0-dim device tensor"""
    return geometry.pose_errors(*_pair("p_mpjpe", predicted, target)).p_mpjpe[0]


def n_mpjpe(predicted, target) -> torch.Tensor:
    """loss.py:68-78, Protocol #3: the mean joint distance after each frame's scale alignment -> 0-dim device tensor"""
    return geometry.pose_errors(*_pair("n_mpjpe", predicted, target)).n_mpjpe[0]


def mean_velocity_error(predicted, target) -> torch.Tensor:
    """loss.py:80-89, MPJVE of one clip [T, J, 3] -> 0-dim device tensor (NaN for T < 2, as the reference's empty mean)"""
    p, g = _dev(predicted), _dev(target)
    if p.dim() != 3 or p.shape[-1] != 3 or p.shape != g.shape:
        raise ValueError(f"mean_velocity_error: need two [T, J, 3] clips, got {list(p.shape)}, {list(g.shape)}")
    return geometry.pose_errors(p, g.to(p.device)).mpjve[0]


def _ragged(name, clips, like=None):
    """a list of [T_i, J, 3] clips -> [B, max T, J, 3] (NaN beyond a clip's length), lengths [B] on the device"""
    clips = [_dev(c, like) for c in clips]
    if not clips:
        raise ValueError(f"{name}: no clips")
    J = clips[0].shape[-2] if clips[0].dim() == 3 else -1
    for c in clips:
        if c.dim() != 3 or c.shape[2] != 3 or c.shape[1] != J:
            raise ValueError(f"{name}: every clip must be [T, {J}, 3], got {list(c.shape)}")
    T = max(int(c.shape[0]) for c in clips)
    X = torch.full((len(clips), T, J, 3), float("nan"), dtype=torch.float64, device=clips[0].device)
    for b, c in enumerate(clips):
        X[b, :c.shape[0]] = c
    return X, [int(c.shape[0]) for c in clips]


def evaluate_clips(preds, targets, zero_root=0):
    """run.py:998-1041, the four numbers `evaluate()` prints: preds, targets lists of [T_i, J, 3] clips (metres) ->
    (e1, e2, e3, ev) = MPJPE, P-MPJPE, N-MPJPE, MPJVE in millimetres, 0-dim device tensors: sum_i T_i metric_i / sum_i T_i
    x 1000, including the reference's quirk that MPJVE is weighted by T_i and not T_i - 1.  zero_root: the target joint that
    counts as the origin (`inputs_3d[:, :, 0] = 0`, :994), None for none.  One pose_errors call over the ragged batch, then
    torch ops on the device; float64 where the reference runs float32."""
    P, lens = _ragged("evaluate_clips", preds)
    G, lens_g = _ragged("evaluate_clips", targets, P)
    if lens != lens_g or P.shape != G.shape:
        raise ValueError("evaluate_clips: preds and targets differ in their shapes")
    r = geometry.pose_errors(P, G, lengths=lens, zero_root=zero_root)
    return weighted_mm(torch.tensor(lens, dtype=torch.float64, device=P.device), (r.mpjpe, r.p_mpjpe, r.n_mpjpe, r.mpjve))


def weighted_mm(frames: torch.Tensor, metrics):
    """run.py:999-1041: every clip's metric weighted by its frame count, in millimetres: sum_i T_i m_i / sum_i T_i x 1000"""
    N = frames.sum()
    return tuple((frames * m).sum() / N * 1000.0 for m in metrics)


FUSED_METRIC_KEYS = ("L-R MeanDist (Before)", "Fused-Left MeanDist", "Fused-Right MeanDist", "L/R→Fused Gain (approx)",
                     "Bone Length CV", "LR Length Symmetry", "Speed P95", "Accel P95", "Symmetry Score (mirror)")


def eval_fused_pose(left_3d, right_3d, fused_3d) -> dict:
    """fuse_eval.eval_fused_pose: left, right, fused [T, 17, 3] or [17, 3] (device tensors or host arrays) -> dict of floats
    with the reference's keys in the reference's order ("Speed P95" / "Accel P95" absent below 3 frames).  One
    geometry.pose_errors call on the three pairs stacked as a batch, one geometry.clip_quality call on the fused clip, and
    one read-back at the end."""
    L = _dev(left_3d)
    R, F = _dev(right_3d, L), _dev(fused_3d, L)
    if L.dim() == 2:
        L, R, F = L[None], R[None] if R.dim() == 2 else R, F[None] if F.dim() == 2 else F
    if L.dim() != 3 or L.shape != R.shape or L.shape != F.shape:
        raise ValueError(f"Shape mismatch: {tuple(L.shape)} vs {tuple(R.shape)} vs {tuple(F.shape)}")
    e = geometry.pose_errors(torch.stack([L, F, F]), torch.stack([R, L, R]))
    q = geometry.clip_quality(F)
    v = torch.cat([e.mpjpe, q.scalars[0]]).cpu().numpy()
    before, f_l, f_r = (float(x) for x in v[:3])
    s = {k: float(x) for k, x in zip(("cv", "cv_mean", "lr", "speed", "jerk", "v95", "a95", "mirror"), v[3:])}
    m = {FUSED_METRIC_KEYS[0]: before, FUSED_METRIC_KEYS[1]: f_l, FUSED_METRIC_KEYS[2]: f_r,
         FUSED_METRIC_KEYS[3]: before - 0.5 * (f_l + f_r), FUSED_METRIC_KEYS[4]: s["cv"], FUSED_METRIC_KEYS[5]: s["lr"]}
    if F.shape[0] >= 3:
        m[FUSED_METRIC_KEYS[6]] = s["v95"]
        m[FUSED_METRIC_KEYS[7]] = s["a95"]
    m[FUSED_METRIC_KEYS[8]] = s["mirror"]
    return m


def format_fused_metrics(metrics: dict) -> str:
    """VideoPose3D/main.py:98-102: the text of fused_metrics.txt"""
    return FUSED_METRICS_HEADER + "\n" + "".join(f"{k:25s}: {v:.4f}\n" for k, v in metrics.items())


def write_fused_metrics(path, metrics: dict) -> Path:
    path = Path(path)
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(format_fused_metrics(metrics), encoding="utf-8")
    return path


def joint_error_summary(pred, target, target_ids=None) -> dict:
    """unity_data_compare.py's calculate_per_joint_errors over a clip + summarize_joint_errors: pred, target [T, J, 3] ->
    {joint id: {"mean", "std", "median", "n"}} over the joint's finite errors (n = 0: three NaN); target_ids names the J
    joints (default 0 .. J - 1).  One pose_errors call, one read-back."""
    p = _dev(pred)
    g = _dev(target, p)
    if p.dim() != 3 or p.shape != g.shape:
        raise ValueError(f"joint_error_summary: need two [T, J, 3] clips, got {list(p.shape)}, {list(g.shape)}")
    J = int(p.shape[1])
    ids = list(range(J)) if target_ids is None else [int(i) for i in target_ids]
    if len(ids) != J:
        raise ValueError(f"joint_error_summary: {len(ids)} target_ids for {J} joints")
    r = geometry.pose_errors(p, g)
    v = torch.cat([r.joint_err[0], r.joint_err_n[0].to(torch.float64)[:, None]], dim=1).cpu().numpy()
    return {jid: {"mean": float(v[j, 0]), "std": float(v[j, 1]), "median": float(v[j, 2]), "n": int(v[j, 3])} for j, jid in enumerate(ids)}


def safe_pct_improvement(baseline: float, target: float) -> float:
    """true_data_compare.py:288-300"""
    if not math.isfinite(baseline) or baseline == 0 or not math.isfinite(target):
        return float("nan")
    return (baseline - target) / baseline * 100.0


def smoothing_gain(raw, smoothed, edges=None) -> dict:
    """The ground-truth-free part of true_data_compare.evaluate_person (:382-419): raw, smoothed [T, J, 3] -> raw_/smooth_
    speed, jerk and bone_cv and the three safe_pct_improvement percentages.  edges: the bones of the CV, default the
    reference's BONE_EDGES for J = 15 (geometry.MHR70_15_EDGES) and the Human3.6M bones for J = 17.  One clip_quality call on
    the two clips as a batch, one read-back."""
    a = _dev(raw)
    b = _dev(smoothed, a)
    if a.dim() != 3 or a.shape != b.shape:
        raise ValueError(f"smoothing_gain: need two [T, J, 3] clips, got {list(a.shape)}, {list(b.shape)}")
    J = int(a.shape[1])
    if edges is None:
        if J not in (15, 17):
            raise ValueError(f"smoothing_gain: no default bones for {J} joints, pass edges")
        edges = geometry.MHR70_15_EDGES if J == 15 else geometry.H36M_EDGES
    q = geometry.clip_quality(torch.stack([a, b]), edges=edges, left_edges=(), right_edges=(), lr_pairs=())
    v = torch.stack([q.speed_mean, q.jerk_mean, q.bone_cv_mean]).cpu().numpy()
    out = {"raw_speed": float(v[0, 0]), "smooth_speed": float(v[0, 1]), "raw_jerk": float(v[1, 0]), "smooth_jerk": float(v[1, 1]),
           "raw_bone_cv": float(v[2, 0]), "smooth_bone_cv": float(v[2, 1])}
    out["jerk_gain_pct"] = safe_pct_improvement(out["raw_jerk"], out["smooth_jerk"])
    out["speed_gain_pct"] = safe_pct_improvement(out["raw_speed"], out["smooth_speed"])
    out["bone_cv_gain_pct"] = safe_pct_improvement(out["raw_bone_cv"], out["smooth_bone_cv"])
    return out
