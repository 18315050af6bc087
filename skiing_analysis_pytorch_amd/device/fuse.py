"""Left/right pose fusion, camera-group fusion, joint quality and temporal smoothing of a clip on the device (csrc/fuse.hip;
C-ABI: skimi_fuse_h36m, skimi_fuse_views, skimi_fuse_group, skimi_joint_quality, skimi_smooth_ema, skimi_smooth_ema_batch,
skimi_smooth_savgol): VideoPose3D/fuse/fuse.py, fuse/main_raw.py:194-250, fuse/main_unity.py:98-132, fuse/fuse.py:124-412;
the host form is the package's fuse.py; rules: DESIGN §2 "Fusion + smoothing on the device", "Group fusion", "Joint
quality".
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch

from .._args import add_lead, f64, f64_dev, i32, strip_lead, upload_f64, workspace
from .._lib import check, current_stream, lib, ptr

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


def fuse_h36m(left_3d: torch.Tensor, right_3d: torch.Tensor, tau=0.08, allow_scale: bool = False, mirror_right_x: bool = False,
              wL=None, wR=None) -> FuseH36MResult:
    """fuse.fuse_pose_no_extrinsics_h36m for a whole clip in one launch: left_3d, right_3d [T, 17, 3] (or [17, 3]) device
    tensors; tau a number or [17]; wL, wR None, [17] or [T, 17] -> FuseH36MResult.  Where the host raises ValueError (fewer
    than 3 torso joints finite on both sides) the frame is NaN and its status False.  mean_gain and bad_frames are torch
    ops on the device: nothing is read back."""
    L, R = f64_dev("fuse_h36m", left_3d), f64_dev("fuse_h36m", right_3d)
    L, R = add_lead(L, 3)[0], add_lead(R, 3)[0]
    if L.shape != R.shape or L.dim() != 3 or tuple(L.shape[1:]) != (17, 3):
        raise ValueError(f"fuse_h36m: inputs must both be (*, 17, 3), got {list(L.shape)}, {list(R.shape)}")
    T, dev = L.shape[0], L.device
    tau_s, tau_j = (float(tau), None) if isinstance(tau, (float, int)) else (0.0, upload_f64(tau, dev))
    if tau_j is not None and tuple(tau_j.shape) != (17,):
        raise ValueError(f"fuse_h36m: tau must be a number or [17], got {list(tau_j.shape)}")

    def weights(w, name):
        if w is None:
            return None, 0
        w = upload_f64(w, dev)
        if tuple(w.shape) not in ((17,), (T, 17)):
            raise ValueError(f"fuse_h36m: {name} must be [17] or [{T}, 17], got {list(w.shape)}")
        return w, 17 if w.dim() == 2 else 0

    (wl, sl), (wr, sr) = weights(wL, "wL"), weights(wR, "wR")
    fused, Rm, tv, s, diag, status = f64(dev, T, 17, 3), f64(dev, T, 3, 3), f64(dev, T, 3), f64(dev, T), f64(dev, T, 4), i32(dev, T)
    check(lib().skimi_fuse_h36m(ptr(L), ptr(R), T, tau_s, ptr(tau_j), ptr(wl), sl, ptr(wr), sr, int(bool(allow_scale)),
                                int(bool(mirror_right_x)), ptr(fused), ptr(Rm), ptr(tv), ptr(s), ptr(diag), ptr(status),
                                current_stream()), "skimi_fuse_h36m")
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
    Xl, Xr, Ul, Ur = (f64_dev("fuse_views", a) for a in (X_l, X_r, U_l, U_r))
    if scale_mode not in FUSE_SCALE_MODES:
        raise ValueError("scale_mode must be 'hip' or 'torso'")
    if Xl.dim() != 3 or Xl.shape[2] != 3 or Xr.shape != Xl.shape or tuple(Ul.shape) != (*Xl.shape[:2], 2) or Ur.shape != Ul.shape:
        raise ValueError(f"fuse_views: need X_l, X_r [T, J, 3] and U_l, U_r [T, J, 2], got {list(Xl.shape)}, {list(Xr.shape)}, "
                         f"{list(Ul.shape)}, {list(Ur.shape)}")
    T, J, dev = Xl.shape[0], Xl.shape[1], Xl.device
    fused, aligned = f64(dev, T, J, 3), f64(dev, T, J, 3)
    per_joint = [f64(dev, T, J) for _ in range(8)]
    fit_ok = i32(dev, T, 2)
    check(lib().skimi_fuse_views(ptr(Xl), ptr(Xr), ptr(Ul), ptr(Ur), T, J, int(root_idx), int(left_hip_idx), int(right_hip_idx),
                                 int(left_shoulder_idx), int(right_shoulder_idx), float(sigma_px), float(sigma_3d),
                                 FUSE_SCALE_MODES[scale_mode], int(min_points), ptr(fused), ptr(aligned), *map(ptr, per_joint),
                                 ptr(fit_ok), current_stream()), "skimi_fuse_views")
    return FuseViewsResult(fused, aligned, *per_joint, fit_ok.bool())


def _clip(fn, X):
    X = f64_dev(fn, X)
    if X.dim() != 3 or X.shape[2] != 3:
        raise ValueError(f"{fn}: need X [T, J, 3], got {list(X.shape)}")
    return X, X.shape[0], X.shape[1]


def smooth_ema(X: torch.Tensor, target_ids=None, alpha: float = 0.7, adaptive: bool = True, alpha_min: float = 0.45,
               alpha_max: float = 0.92, speed_gain: float = 0.25) -> EmaResult:
    """fuse.temporal_smooth_ema on the device: X [T, J, 3] (NaN rows = missing joints) -> EmaResult.  One thread per joint
    walks the clip; the per-joint base factors come from alpha, target_ids and fuse._ALPHA_FACTOR as on the host.
    X [B, T, J, 3] smooths B clips in one launch (skimi_smooth_ema_batch): clip b's result is the [T, J, 3] call's on X[b] bit
    for bit; B = 0 is accepted."""
    from .. import fuse

    X = f64_dev("smooth_ema", X)
    batched = X.dim() == 4
    if X.dim() not in (3, 4) or X.shape[-1] != 3:
        raise ValueError(f"smooth_ema: need X [T, J, 3] or [B, T, J, 3], got {list(X.shape)}")
    T, J = X.shape[-3], X.shape[-2]
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
    if batched:
        check(lib().skimi_smooth_ema_batch(ptr(X), X.shape[0], T, J, ptr(base), int(bool(adaptive)), float(alpha_min),
                                           float(alpha_max), float(speed_gain), ptr(Y), current_stream()), "skimi_smooth_ema_batch")
    else:
        check(lib().skimi_smooth_ema(ptr(X), T, J, ptr(base), int(bool(adaptive)), float(alpha_min), float(alpha_max),
                                     float(speed_gain), ptr(Y), current_stream()), "skimi_smooth_ema")
    return EmaResult(Y, base)


_savgol_ops = {}   # (win, poly, device) -> the three operators on the device


def smooth_savgol(X: torch.Tensor, win: int = 9, poly: int = 2) -> SavgolResult:
    """fuse.smooth_skeleton on the device: X [T, J, 3] -> SavgolResult.  The window is the reference's min(odd(win), max(1
    if T is odd else T - 1, 3)); every (joint, coordinate) series with at least that many finite samples is filtered over
    them as one contiguous series, everything else passes through bit for bit.  The window must not exceed 33 and must
    exceed poly (the host raises for poly >= window only once a series is long enough to be filtered)."""
    from .. import fuse

    X, T, J = _clip("smooth_savgol", X)
    w = fuse.savgol_window(T, int(win))
    Y = torch.empty_like(X)
    key = (w, int(poly), X.device)
    if key not in _savgol_ops and 1 <= w <= SAVGOL_MAX_WIN and 0 <= int(poly) < w:
        _savgol_ops[key] = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(X.device) for a in fuse.savgol_operators(w, int(poly)))
    fir, first, last = _savgol_ops.get(key, (None, None, None))     # a refused (win, poly) has none: the library says why
    check(lib().skimi_smooth_savgol(ptr(X), T, J, w, int(poly), ptr(fir), ptr(first), ptr(last), ptr(Y), current_stream()),
          "skimi_smooth_savgol")
    return SavgolResult(Y, w)


class FuseGroupResult(NamedTuple):
    """fuse_group's outputs (device tensors; V views, P = V (V - 1) / 2 pairs, T frames, J joints).  With given qualities the
    confidence outputs (conf_x, dist, conf, err, fit_ok) are None."""
    pairs: torch.Tensor       # int32 [P, 2]: (a, b), a < b, in itertools.combinations order
    fused: torch.Tensor       # float64 [P, T, J, 3]
    aligned: torch.Tensor     # float64 [P, T, J, 3]: view b in view a's frame (align=True), else view b itself
    q_a: torch.Tensor         # float64 [P, T, J]
    q_b: torch.Tensor
    conf_x: torch.Tensor      # float64 [P, T, J]: cross-view consistency confidence
    dist: torch.Tensor        # float64 [P, T, J]
    conf: torch.Tensor        # float64 [V, T, J]: weak-perspective reprojection confidence of each view
    err: torch.Tensor         # float64 [V, T, J]
    fit_ok: torch.Tensor      # bool [V, T]


def fuse_group(X: torch.Tensor, U, *, root_idx: int, left_hip_idx: int, right_hip_idx: int, left_shoulder_idx: int,
               right_shoulder_idx: int, sigma_px: float = 12.0, sigma_3d: float = 0.08, scale_mode: str = "hip", min_points: int = 8,
               align: bool = False, quality="confidence") -> FuseGroupResult:
    """Every pair of a camera group fused in one call: X [V, T, J, 3], U [V, T, J, 2] device tensors -> FuseGroupResult.
    align=False is fuse/main_unity.py's _fuse_pair (fuse_frame_3d on the raw poses), align=True fuse/main_raw.py's frame body
    (view b Kabsch-aligned onto view a first; pair (a, b) then equals fuse_views(X[a], X[b], U[a], U[b]) bit for bit).
    quality="confidence": q = sqrt(conf conf_x), each view's weak-perspective fit and canonical pose computed once;
    quality=<tensor [V, T, J]> (joint_quality(...).q, say): those qualities, U may be None, no confidences."""
    X = f64_dev("fuse_group", X)
    if scale_mode not in FUSE_SCALE_MODES:
        raise ValueError("scale_mode must be 'hip' or 'torso'")
    if X.dim() != 4 or X.shape[3] != 3:
        raise ValueError(f"fuse_group: need X [V, T, J, 3], got {list(X.shape)}")
    V, T, J, dev = X.shape[0], X.shape[1], X.shape[2], X.device
    given = not isinstance(quality, str)
    if not given and quality != "confidence":
        raise ValueError("fuse_group: quality must be 'confidence' or a [V, T, J] tensor")
    Q = f64_dev("fuse_group", quality, dev) if given else None
    Ud = None if (given and U is None) else f64_dev("fuse_group", U, dev)
    if Ud is not None and tuple(Ud.shape) != (V, T, J, 2):
        raise ValueError(f"fuse_group: U must be [{V}, {T}, {J}, 2], got {list(Ud.shape)}")
    if Q is not None and tuple(Q.shape) != (V, T, J):
        raise ValueError(f"fuse_group: quality must be [{V}, {T}, {J}], got {list(Q.shape)}")
    pairs = torch.tensor([(a, b) for a in range(V) for b in range(a + 1, V)], dtype=torch.int32).reshape(-1, 2).to(dev)
    P = pairs.shape[0]
    fused, aligned, q_a, q_b = f64(dev, P, T, J, 3), f64(dev, P, T, J, 3), f64(dev, P, T, J), f64(dev, P, T, J)
    conf_x = dist = conf = err = fit_ok = ws = None
    nbytes = 0
    if not given:
        conf_x, dist, conf, err, fit_ok = f64(dev, P, T, J), f64(dev, P, T, J), f64(dev, V, T, J), f64(dev, V, T, J), i32(dev, V, T)
        nbytes = int(lib().skimi_fuse_group_workspace_bytes(V, T, J))
        ws = workspace(dev, nbytes, at_least=8, as_f64=True)
    check(lib().skimi_fuse_group(ptr(X), ptr(Ud), ptr(Q), V, T, J, int(root_idx), int(left_hip_idx), int(right_hip_idx),
                                 int(left_shoulder_idx), int(right_shoulder_idx), float(sigma_px), float(sigma_3d),
                                 FUSE_SCALE_MODES[scale_mode], int(min_points), int(bool(align)), ptr(ws), nbytes, ptr(fused),
                                 ptr(aligned), ptr(q_a), ptr(q_b), ptr(conf_x), ptr(dist), ptr(conf), ptr(err), ptr(fit_ok),
                                 current_stream()), "skimi_fuse_group")
    return FuseGroupResult(pairs, fused, aligned, q_a, q_b, conf_x, dist, conf, err, None if given else fit_ok.bool())


class JointQualityResult(NamedTuple):
    """joint_quality's outputs (device tensors; V views, T frames, J joints, E edges; without the view axis for a [T, J, 3]
    input)."""
    q: torch.Tensor           # float64 [V, T, J]
    q_bone: torch.Tensor      # float64 [V, T, J]: -1e9 missing joint, -100 no usable edge
    q_temp: torch.Tensor      # float64 [V, T, J]
    q_san: torch.Tensor       # float64 [V, T, J]: 0 or -50
    med_lens: torch.Tensor    # float64 [V, E]


def joint_quality(X: torch.Tensor, U=None, *, edges, size, beta_temp: float = 1.0, w_bone: float = 1.0, w_temp: float = 0.3,
                  w_san: float = 0.2, med_lens=None, bias=None) -> JointQualityResult:
    """The ground-truth-free joint quality of fuse/fuse.py:124-285 (fuse.compute_q_nogt on the host) for V clips: X [V, T, J,
    3] ([T, J, 3]: V = 1) device tensor, NaN rows = missing joints; U [V, T, J, 2] or None; edges [E, 2] positions on the
    joint axis; size (width, height), shared or one per view; med_lens [V, E]: used instead of the clips' medians; bias
    [J] or [V, J]: added at the end (+b for the left camera, -b for the right one) -> JointQualityResult."""
    X, single = add_lead(f64_dev("joint_quality", X), 4)
    if X.dim() != 4 or X.shape[3] != 3:
        raise ValueError(f"joint_quality: need X [V, T, J, 3] or [T, J, 3], got {list(X.shape)}")
    V, T, J, dev = X.shape[0], X.shape[1], X.shape[2], X.device
    Ud = None
    if U is not None:
        Ud = add_lead(f64_dev("joint_quality", U, dev), 4)[0] if single else f64_dev("joint_quality", U, dev)
        if tuple(Ud.shape) != (V, T, J, 2):
            raise ValueError(f"joint_quality: U must be [{V}, {T}, {J}, 2], got {list(Ud.shape)}")
    ed = edges if isinstance(edges, torch.Tensor) else torch.as_tensor(np.asarray(list(edges), dtype=np.int64).reshape(-1, 2))
    if ed.dim() != 2 or ed.shape[1] != 2:
        raise ValueError(f"joint_quality: edges must be [E, 2], got {list(ed.shape)}")
    ed = ed.to(dev, torch.int32).contiguous()
    E = ed.shape[0]
    sz = np.asarray(size, dtype=np.float64)
    if sz.shape not in ((2,), (V, 2)):
        raise ValueError(f"joint_quality: size must be (width, height) or [{V}, 2], got {list(sz.shape)}")
    sz = torch.from_numpy(np.broadcast_to(sz, (V, 2)).copy(order="C")).to(dev).contiguous()      # broadcast views are read-only
    if med_lens is None:
        med = f64(dev, V, E)
    else:
        med = upload_f64(med_lens, dev)
        med = med[None] if single and med.dim() == 1 else med
        if tuple(med.shape) != (V, E):
            raise ValueError(f"joint_quality: med_lens must be [{V}, {E}], got {list(med.shape)}")
    b, bs = None, 0
    if bias is not None:
        b = upload_f64(bias, dev)
        if tuple(b.shape) not in ((J,), (V, J)):
            raise ValueError(f"joint_quality: bias must be [{J}] or [{V}, {J}], got {list(b.shape)}")
        bs = J if b.dim() == 2 else 0
    q, qb, qt, qs = (f64(dev, V, T, J) for _ in range(4))
    check(lib().skimi_joint_quality(ptr(X), ptr(Ud), V, T, J, ptr(ed), E, ptr(sz), float(beta_temp), float(w_bone), float(w_temp),
                                    float(w_san), int(med_lens is not None), ptr(b), bs, ptr(med), ptr(q), ptr(qb), ptr(qt), ptr(qs),
                                    current_stream()), "skimi_joint_quality")
    return JointQualityResult(*strip_lead((q, qb, qt, qs, med), single))
