"""Seeded inputs of tests/test_fuse_device_cpu.py and tests/test_fuse_device_gpu.py, and the host side of the comparison:
the functions of skiing_analysis_pytorch_amd/fuse.py (pinned to the reference by tests/golden/fuse_ema.npz and
fuse_align.npz) applied frame by frame, with the two rules the device build sets where the host raises.  Every host
result is computed once per process and shared."""
import functools

import numpy as np

from skiing_analysis_pytorch_amd import fuse

NAN = np.nan
TORSO = fuse.H36M_TORSO

# a rough H36M-17 body (metres; x to the subject's left, y up): the torso joints 0, 1, 4, 9, 11, 14 lie close to a plane
_H36M_BODY = np.array([
    [0.00, 0.00, 0.00], [-0.13, 0.00, 0.02], [-0.14, -0.45, 0.04], [-0.14, -0.90, 0.00], [0.13, 0.00, -0.02],
    [0.14, -0.45, 0.05], [0.14, -0.90, 0.01], [0.00, 0.25, 0.02], [0.00, 0.50, 0.03], [0.00, 0.60, 0.06],
    [0.00, 0.72, 0.05], [0.18, 0.48, 0.00], [0.30, 0.22, 0.02], [0.33, 0.00, 0.10], [-0.18, 0.48, 0.02],
    [-0.30, 0.22, 0.03], [-0.33, 0.00, 0.11]])


def _rot_y(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])


def _walk(rng, body, T, amp=0.05):
    """[T, J, 3]: the body with a smooth motion per joint coordinate and a smooth drift of the whole"""
    J = body.shape[0]
    t = np.arange(T)[:, None, None] / 30.0
    f = rng.uniform(0.5, 2.0, size=(1, J, 3))
    ph = rng.uniform(0, 2 * np.pi, size=(1, J, 3))
    drift = np.stack([0.8 * t[:, 0, 0], 0.05 * np.sin(3.0 * t[:, 0, 0]), 0.3 * t[:, 0, 0]], axis=1)[:, None, :]
    return body[None] + amp * np.sin(2 * np.pi * f * t + ph) + drift


def _other_view(rng, L, noise=0.02):
    """right = left rotated by about 1.1 rad about y, scaled 1.07, shifted, plus noise"""
    Rm = _rot_y(1.1) @ _rot_y(0.0)
    return 1.07 * (L @ Rm.T) + np.array([0.4, -0.1, 2.0]) + noise * rng.normal(size=L.shape)


def _h36m_pair(seed, T):
    rng = np.random.default_rng(seed)
    body = _H36M_BODY + 0.03 * rng.normal(size=_H36M_BODY.shape)
    L = _walk(rng, body, T)
    return rng, L, _other_view(rng, L)


# frames of the T = 67 clip with something special
F_NAN_LEFT, F_NAN_BOTH, F_NAN_TORSO, F_NAN_PELVIS, F_TWO_TORSO, F_MIRRORED, F_PLANAR = 3, 5, 7, 9, 11, 13, 15


@functools.lru_cache(maxsize=None)
def h36m_cases():
    """name -> dict(left, right [T, 17, 3], kw of fuse_pose_no_extrinsics_h36m / geometry.fuse_h36m)"""
    cases = {}
    _, L, R = _h36m_pair(1, 1)
    cases["T1"] = dict(left=L, right=R, kw=dict(tau=0.08))
    rng, L, R = _h36m_pair(2, 2)
    cases["T2_tau17"] = dict(left=L, right=R, kw=dict(tau=rng.uniform(0.03, 0.12, size=17)))
    rng, L, R = _h36m_pair(3, 67)
    L[F_NAN_LEFT, 13] = NAN                         # a non-torso joint on one side
    L[F_NAN_BOTH, 6] = NAN                          # the same joint on both sides
    R[F_NAN_BOTH, 6] = NAN
    R[F_NAN_TORSO, 11, 1] = NAN                     # a torso joint: the fit runs on 5 rows
    L[F_NAN_PELVIS, 0] = NAN                        # the pelvis: everything of the frame is NaN
    R[F_TWO_TORSO, [4, 1, 11, 14]] = NAN            # 2 finite torso rows left
    R[F_MIRRORED, :, 0] *= -1.0                     # a mirrored right view: det < 0
    # a near-planar torso: the torso joints pressed into the plane z = 0 of the left view, the right view made from it
    flat = L[F_PLANAR].copy()
    flat[TORSO, 2] = flat[0, 2] + 0.004 * rng.normal(size=6)
    L[F_PLANAR] = flat
    R[F_PLANAR] = _other_view(rng, flat, noise=0.002)
    cases["T67_mixed_w17"] = dict(left=L, right=R, kw=dict(tau=0.08, wL=rng.uniform(0.2, 1.0, size=17), wR=rng.uniform(0.2, 1.0, size=17)))
    cases["T67_mixed_ref"] = dict(left=L, right=R, kw=dict(tau=0.06, allow_scale=False, mirror_right_x=False))
    rng, L, R = _h36m_pair(4, 243)
    R[:, :, 0] *= -1.0                               # undone by mirror_right_x up to a rotation about y
    R[:, :, 2] *= -1.0
    cases["T243_scale_mirror_wT17"] = dict(left=L, right=R, kw=dict(tau=0.08, allow_scale=True, mirror_right_x=True,
                                                                   wL=rng.uniform(0.2, 1.0, size=(243, 17)),
                                                                   wR=rng.uniform(0.2, 1.0, size=(243, 17))))
    return cases


def host_h36m(left, right, kw):
    """fuse.fuse_pose_no_extrinsics_h36m frame by frame -> dict of arrays as geometry.fuse_h36m returns them; a frame for which
    the host raises (fewer than 3 torso rows finite on both sides) is NaN with status 0, the rule of the device build"""
    T = left.shape[0]
    out = dict(fused=np.full((T, 17, 3), NAN), R=np.full((T, 3, 3), NAN), t=np.full((T, 3), NAN), s=np.full(T, NAN),
               diag=np.full((T, 4), NAN), status=np.zeros(T, dtype=bool), det=np.full(T, NAN), dist_tau=np.full((T, 17), NAN))
    kw = dict(kw)
    wL, wR = kw.pop("wL", None), kw.pop("wR", None)
    for t in range(T):
        w = {k: (None if v is None else (v if np.ndim(v) == 1 else v[t])) for k, v in (("wL", wL), ("wR", wR))}
        try:
            fused, diag = fuse.fuse_pose_no_extrinsics_h36m(left[t], right[t], **kw, **w)
        except ValueError:
            continue
        d = diag["per_frame"][0]
        out["fused"][t], out["R"][t], out["t"][t], out["s"][t] = fused, d["R"], d["t"], d["s"]
        out["diag"][t] = [d["LR_before"], d["Fused_vs_L"], d["Fused_vs_R"], d["gain"]]
        out["status"][t] = True
        # what the branches hang on: det(U V^T) before the flip and ||L - R_aligned|| - tau per joint
        Rt = right[t].copy()
        if kw.get("mirror_right_x", False):
            Rt[:, 0] *= -1
            Rt[:, 2] *= -1
        Ln, Rn = fuse.center_scale_h36m(left[t].copy())[0], fuse.center_scale_h36m(Rt)[0]
        ok = np.isfinite(Ln[TORSO]).all(1) & np.isfinite(Rn[TORSO]).all(1)
        X, Y = Ln[TORSO][ok], Rn[TORSO][ok]
        U, S, Vt = np.linalg.svd((Y - Y.mean(0)).T @ (X - X.mean(0)) / len(X))
        out["det"][t] = np.linalg.det(U @ Vt)
        out.setdefault("sv", np.full((T, 3), NAN))[t] = S
        al = d["s"] * (d["R"] @ Rn.T).T + d["t"]
        tau = kw.get("tau", 0.08)
        out["dist_tau"][t] = np.linalg.norm(Ln - al, axis=1) - (np.full(17, float(tau)) if np.ndim(tau) == 0 else tau)
    return out


@functools.lru_cache(maxsize=None)
def host_h36m_case(name):
    c = h36m_cases()[name]
    return host_h36m(c["left"], c["right"], c["kw"])


# ---- two-view clips ---------------------------------------------------------------------------------------------------
KEYS70 = dict(root_idx=0, left_hip_idx=9, right_hip_idx=10, left_shoulder_idx=5, right_shoulder_idx=6)
KEYS17 = dict(root_idx=0, left_hip_idx=4, right_hip_idx=1, left_shoulder_idx=11, right_shoulder_idx=14)
V_NAN_3D, V_NAN_2D, V_FEW_COMMON, V_FEW_FIT, V_NO_KEY = 2, 4, 6, 8, 10


def _project(rng, X, noise=3.0):
    """pinhole keypoints of camera-frame points standing about 8 m away, plus pixel noise.  The crop's principal point is
    close to the origin: a residual is a difference of pixel coordinates, and a 1e-13 relative change of coordinates in
    the hundreds would move a sub-pixel residual by more than the 1e-10 the stability condition allows"""
    Z = X[..., 2] + 8.0
    u = 1000.0 * X[..., 0] / Z + 64.0
    v = 1000.0 * X[..., 1] / Z + 36.0
    return np.stack([u, v], axis=-1) + noise * rng.normal(size=X.shape[:-1] + (2,))


def _views_pair(seed, T, J):
    rng = np.random.default_rng(seed)
    body = _H36M_BODY + 0.03 * rng.normal(size=(17, 3)) if J == 17 else rng.uniform(-0.5, 0.5, size=(J, 3)) * np.array([0.6, 1.8, 0.4])
    Xl = _walk(rng, body, T, amp=0.04)
    Xl -= Xl[:, :1].mean(axis=0, keepdims=True)      # the clip stays in front of the camera
    Xr = 1.03 * (Xl @ _rot_y(0.9).T) + np.array([0.1, 0.05, 0.3]) + 0.02 * rng.normal(size=Xl.shape)
    return rng, Xl, Xr, _project(rng, Xl), _project(rng, Xr)


@functools.lru_cache(maxsize=None)
def views_cases():
    """name -> dict(Xl, Xr [T, J, 3], Ul, Ur [T, J, 2], kw of geometry.fuse_views)"""
    cases = {}
    _, Xl, Xr, Ul, Ur = _views_pair(11, 1, 70)
    cases["J70_T1"] = dict(Xl=Xl, Xr=Xr, Ul=Ul, Ur=Ur, kw=dict(**KEYS70, sigma_px=12.0, sigma_3d=0.08, scale_mode="hip", min_points=8))
    rng, Xl, Xr, Ul, Ur = _views_pair(12, 65, 70)
    Xl[V_NAN_3D, [3, 17, 64, 69]] = NAN             # NaN 3D joints, one of them on both sides, lanes of both halves
    Xr[V_NAN_3D, [17, 30, 65]] = NAN
    Ul[V_NAN_2D, [2, 40, 68]] = NAN                 # NaN 2D joints
    Ur[V_NAN_2D, 41, 0] = NAN
    Xl[V_FEW_COMMON, 2:] = NAN                      # 2 common joints: the right view stays as it is
    Ul[V_FEW_FIT, 7:] = NAN                         # 7 fit points in the left view
    Xr[V_NO_KEY, 10] = NAN                          # a key joint missing: the cross-view confidence is 0
    cases["J70_T65_mixed"] = dict(Xl=Xl, Xr=Xr, Ul=Ul, Ur=Ur, kw=dict(**KEYS70, sigma_px=12.0, sigma_3d=0.08, scale_mode="hip", min_points=8))
    cases["J70_T65_torso"] = dict(Xl=Xl, Xr=Xr, Ul=Ul, Ur=Ur, kw=dict(**KEYS70, sigma_px=20.0, sigma_3d=0.15, scale_mode="torso", min_points=8))
    rng, Xl, Xr, Ul, Ur = _views_pair(13, 3, 17)
    Xl[1, 13] = NAN
    Ur[2, 3] = NAN
    cases["J17_T3_torso"] = dict(Xl=Xl, Xr=Xr, Ul=Ul, Ur=Ur, kw=dict(**KEYS17, sigma_px=12.0, sigma_3d=0.08, scale_mode="torso", min_points=8))
    return cases


VIEW_FLOATS = ("fused", "aligned", "q_l", "q_r", "conf_l", "conf_r", "conf_x", "err_l", "err_r", "dist")


def host_views(Xl, Xr, Ul, Ur, kw):
    """the per-frame body of fuse/main_raw.py:194-240 with fuse.py's functions -> dict of arrays as geometry.fuse_views
    returns them; a weak-perspective fit for which the host raises gives conf 0, err NaN and fit_ok 0 for that view, the rule
    of the device build.  `det`: the Kabsch determinant before the flip (NaN without a fit)."""
    T, J = Xl.shape[:2]
    out = {k: np.full((T, J, 3) if k in ("fused", "aligned") else (T, J), NAN) for k in VIEW_FLOATS}
    out["fit_ok"] = np.zeros((T, 2), dtype=bool)
    out["det"] = np.full(T, NAN)
    keys = {k: v for k, v in kw.items() if k.endswith("_idx")}
    for t in range(T):
        out["aligned"][t] = al = fuse.align_right_to_left(Xl[t], Xr[t])
        conf = []
        for v, (X, U) in enumerate(((Xl[t], Ul[t]), (Xr[t], Ur[t]))):
            try:
                c, e, _, _ = fuse.weakpersp_reproj_confidence(X, U, sigma_px=kw["sigma_px"], min_points=kw["min_points"])
                out["fit_ok"][t, v] = True
            except ValueError:
                c, e = np.zeros(J), np.full(J, NAN)
            conf.append(c)
            out[("conf_l", "conf_r")[v]][t], out[("err_l", "err_r")[v]][t] = c, e
        cx, d, _, _, _ = fuse.crossview_consistency_confidence(Xl[t], Xr[t], **keys, sigma_3d=kw["sigma_3d"], scale_mode=kw["scale_mode"])
        out["conf_x"][t], out["dist"][t] = cx, d
        out["q_l"][t], out["q_r"][t] = np.sqrt(conf[0] * cx), np.sqrt(conf[1] * cx)
        out["fused"][t] = fuse.fuse_frame_3d(Xl[t], al, out["q_l"][t], out["q_r"][t])
        both = np.isfinite(Xl[t]).all(1) & np.isfinite(Xr[t]).all(1)
        if both.sum() >= 3:
            src, dst = Xr[t][both], Xl[t][both]
            U_, _, Vt = np.linalg.svd((src - src.mean(0)).T @ (dst - dst.mean(0)))
            out["det"][t] = np.linalg.det(Vt.T @ U_.T)
    return out


@functools.lru_cache(maxsize=None)
def host_views_case(name):
    c = views_cases()[name]
    return host_views(c["Xl"], c["Xr"], c["Ul"], c["Ur"], c["kw"])


# ---- smoothing clips --------------------------------------------------------------------------------------------------
SMOOTH_T = (0, 1, 2, 8, 9, 500)
IDS6 = [1, 13, 99, 5, 69, 41]          # the 0.85 factor, the 1.15 factor, out of range, plain, 0.85, 1.15


@functools.lru_cache(maxsize=None)
def smooth_clip(T):
    """[T, J, 3] with NaN rows; J = 6 (T < 500) or 70"""
    rng = np.random.default_rng(100 + T)
    J = 70 if T >= 500 else 6
    X = _walk(rng, rng.uniform(-0.5, 0.5, size=(J, 3)), T, amp=0.08) + 0.01 * rng.normal(size=(T, J, 3))
    if T >= 2:
        X[: max(1, T // 3), 1] = NAN                # appears late
        X[:, 3] = NAN                                # never observed
    if T >= 8:
        X[3:5, 2] = NAN                              # vanishes and returns
        X[T - 2, 2] = NAN
        X[2, 4, 1] = NAN                             # a row with one coordinate missing: not observed, but its x and z are samples
        X[[0] + list(range(2, T - 2)) + [T - 1], 5] = NAN   # two samples: fewer than every window
        X[0, 0, 2] = NAN                             # the first row of a joint incomplete
    if T >= 500:
        X[rng.random(size=(T, J)) < 0.1] = NAN
        X[40:, 7] = NAN                              # 40 steps at most, then gone for good
        X[:, 8] = NAN
        X[[5, 100, 250], 8] = rng.normal(size=(3, 3))   # three samples: under every window
    return X


EMA_VARIANTS = (dict(), dict(adaptive=False, alpha=0.6), dict(target_ids=IDS6, alpha=0.5, alpha_min=0.3, alpha_max=0.6, speed_gain=2.0))
SAVGOL_VARIANTS = (dict(), dict(win=5, poly=3), dict(win=4, poly=1))


def ema_kw(T, variant):
    kw = dict(EMA_VARIANTS[variant])
    if "target_ids" in kw and T >= 500:
        kw["target_ids"] = list(range(35)) + [-1, 70, 1000] + list(range(38, 70))
    return kw


@functools.lru_cache(maxsize=None)
def host_ema(T, variant):
    return fuse.temporal_smooth_ema(smooth_clip(T), **ema_kw(T, variant))


@functools.lru_cache(maxsize=None)
def host_savgol(T, variant):
    return fuse.smooth_skeleton(smooth_clip(T), **SAVGOL_VARIANTS[variant])


def perturbed(rng, *arrays):
    """the arrays scaled element-wise by 1 + 1e-13 N(0, 1)"""
    return [a * (1.0 + 1e-13 * rng.normal(size=a.shape)) for a in arrays]


def close(got, want, tol=1e-9):
    """-> the worst |got - want| / (1 + |want|); raises unless the NaN patterns are equal and that figure is within tol"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), "NaN patterns differ"
    fin = ~np.isnan(want)
    if not fin.any():
        return 0.0
    worst = float(np.max(np.abs(got[fin] - want[fin]) / (1.0 + np.abs(want[fin]))))
    assert worst <= tol, worst
    return worst
