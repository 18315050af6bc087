"""The kinematic analysis of a clip restated in vectorised float64 NumPy from the rules of include/skimi.h (DESIGN §2
"Kinematics"): the 14 base series and the heading, the 28 change series, the turns and the per-turn statistics.  It follows
the rules, not the reference's loops, handles `lengths` and clips shorter than a smoothing window (where the reference
raises), and also returns the quantities every discrete decision hangs on, so that tests can assert their margins.

tests/test_kinematics_cpu.py holds it against the reference's own outputs (tests/golden/kinematics.npz);
tests/test_kinematics_gpu.py holds csrc/kinematics.hip against it."""
import numpy as np

ROLES = ("shoulder_l", "shoulder_r", "elbow_l", "elbow_r", "hip_l", "hip_r", "knee_l", "knee_r", "foot_l", "foot_r", "hand_l",
         "hand_r", "neck")
BASE = ("knee_l", "knee_r", "elbow_l", "elbow_r", "shoulder_l", "shoulder_r", "hip_l", "hip_r", "torso_knee_angle",
        "knee_diff_lr", "elbow_distance_l", "elbow_distance_r", "tilt_upper", "tilt_lower")
SERIES = BASE + tuple(n + s for n in BASE for s in ("_d", "_abs_d"))
# angle ABC of each joint-angle series, as roles
ANGLES = {"knee_l": ("hip_l", "knee_l", "foot_l"), "knee_r": ("hip_r", "knee_r", "foot_r"),
          "elbow_l": ("shoulder_l", "elbow_l", "hand_l"), "elbow_r": ("shoulder_r", "elbow_r", "hand_r"),
          "shoulder_l": ("neck", "shoulder_l", "elbow_l"), "shoulder_r": ("neck", "shoulder_r", "elbow_r"),
          "hip_l": ("neck", "hip_l", "knee_l"), "hip_r": ("neck", "hip_r", "knee_r")}
MHR70_15 = (2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 12, 14)
H36M_17 = (11, 14, 12, 15, 4, 1, 5, 2, 6, 3, 13, 16, 8)
DEG, RAD = 180.0 / np.pi, np.pi / 180.0


def max_turns(frames, min_turn_frames=12):
    return (frames - 1) // min_turn_frames + 1 if frames > 0 else 0


def _fin(p):
    return np.isfinite(p).all(axis=-1)


def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _unit(v):
    """v / |v| and where that exists (a non-zero finite norm)"""
    n = np.sqrt(_dot(v, v))
    ok = (n != 0.0) & np.isfinite(n)
    return v / np.where(ok, n, 1.0)[..., None], ok


def _angle(a, b, c):
    """the angle ABC in degrees and its cosine (NaN where undefined)"""
    ba, bc = a - b, c - b
    na, nc = np.sqrt(_dot(ba, ba)), np.sqrt(_dot(bc, bc))
    ok = _fin(a) & _fin(b) & _fin(c) & (na != 0.0) & (nc != 0.0)
    cos = np.where(ok, _dot(ba, bc) / np.where(ok, na * nc, 1.0), np.nan)
    return np.arccos(np.clip(cos, -1.0, 1.0)) * DEG, cos


def _centre(a, b):
    fa, fb = _fin(a)[:, None], _fin(b)[:, None]
    return np.where(fa & fb, (a + b) / 2.0, np.where(fa, a, np.where(fb, b, np.nan)))


def base_series(X, layout=MHR70_15, up_axis=(0.0, -1.0, 0.0)):
    """X [T, J, 3] -> series [14, T], heading [T], debug dict (cosines [8, T], tilt_dots [2, T])"""
    X = np.asarray(X, dtype=np.float64)
    T = X.shape[0]
    up = np.asarray(up_axis, dtype=np.float64)
    with np.errstate(all="ignore"):
        P = {r: (X[:, j] if j >= 0 else np.full((T, 3), np.nan)) for r, j in zip(ROLES, layout)}
        out, cosines = {}, []
        for name, (a, b, c) in ANGLES.items():
            out[name], cos = _angle(P[a], P[b], P[c])
            cosines.append(cos)
        pelvis, shoulder, knee = _centre(P["hip_l"], P["hip_r"]), _centre(P["shoulder_l"], P["shoulder_r"]), _centre(P["knee_l"], P["knee_r"])
        out["torso_knee_angle"], _ = _angle(shoulder, pelvis, knee)
        out["knee_diff_lr"] = np.where(np.isfinite(out["knee_l"]) & np.isfinite(out["knee_r"]), out["knee_l"] - out["knee_r"], np.nan)
        for side in "lr":
            e = P["elbow_" + side]
            dx, dz = e[:, 0] - pelvis[:, 0], e[:, 2] - pelvis[:, 2]
            out["elbow_distance_" + side] = np.where(_fin(pelvis) & _fin(e), np.sqrt(dx * dx + dz * dz), np.nan)
        hips = _fin(P["hip_l"]) & _fin(P["hip_r"])
        shoulders = _fin(P["shoulder_l"]) & _fin(P["shoulder_r"])
        lr = np.where(hips[:, None], P["hip_r"] - P["hip_l"], P["shoulder_r"] - P["shoulder_l"])
        l, ok_l = _unit(lr)
        u = up / np.sqrt(_dot(up, up))
        f, ok_f = _unit(np.cross(u[None], l) if up[1] < 0 else np.cross(l, u[None]))
        ok = (hips | shoulders) & ok_l & ok_f
        heading = np.where(ok, np.arctan2(f[:, 0], f[:, 2]) * DEG, np.nan)
        dots = []
        for name, top in (("tilt_upper", shoulder), ("tilt_lower", knee)):
            v = top - pelvis
            p = v - _dot(v, l)[:, None] * l
            q, ok_q = _unit(p)
            okv = ok & _fin(v) & _fin(p) & ok_q
            theta = np.arccos(np.clip(_dot(q, u[None]), -1.0, 1.0)) * DEG
            d = _dot(q, f)
            out[name] = np.where(okv, np.where(d >= 0.0, theta, -theta), np.nan)
            dots.append(np.where(okv, d, np.nan))
    series = np.stack([out[n] for n in BASE]) if T else np.zeros((len(BASE), 0))
    return series, heading, dict(cosines=np.stack(cosines), tilt_dots=np.stack(dots))


def changes(series):
    """[14, T] -> [28, T]: name_d, name_abs_d of each series in turn"""
    d = np.full_like(series, np.nan)
    if series.shape[1] > 1:
        prev, cur = series[:, :-1], series[:, 1:]
        with np.errstate(all="ignore"):
            d[:, 1:] = np.where(np.isfinite(prev) & np.isfinite(cur), cur - prev, np.nan)
    return np.stack([d, np.abs(d)], axis=1).reshape(2 * series.shape[0], -1)


def box_mean(x, w):
    """the sum over the samples of i - w/2 .. i + w/2 inside the clip, in ascending order, over their number"""
    n, r = x.shape[0], w // 2
    xp = np.concatenate([np.zeros(r), x, np.zeros(r)])
    cp = np.concatenate([np.zeros(r), np.ones(n), np.zeros(r)])
    s, c = np.zeros(n), np.zeros(n)
    for j in range(w):
        s = s + xp[j:j + n]
        c = c + cp[j:j + n]
    return s / c


def turns(heading, min_turn_frames=12, min_heading_change_deg=8.0, heading_window=11, velocity_window=9):
    """heading [T] (degrees) -> heading_smooth [T], velocity_smooth [T], list of (start, end, heading change), debug dict (dd
    [T - 1], extrema, segments = every (start, end, heading change) before the filter)"""
    h = np.asarray(heading, dtype=np.float64)
    T = h.shape[0]
    nan = np.full(T, np.nan)
    ok = np.isfinite(h)
    if ok.sum() < 5:
        return nan, nan.copy(), [], dict(dd=np.zeros(0), extrema=np.zeros(0, dtype=np.int64), segments=[])
    idx = np.arange(T)
    left = np.maximum.accumulate(np.where(ok, idx, -1))
    right = np.minimum.accumulate(np.where(ok, idx, T)[::-1])[::-1]
    hl, hr = h[np.maximum(left, 0)], h[np.minimum(right, T - 1)]
    with np.errstate(all="ignore"):
        between = (hr - hl) / np.maximum(right - left, 1) * (idx - left) + hl
    filled = np.where(ok, h, np.where(left < 0, hr, np.where(right >= T, hl, between)))
    p = filled * RAD
    dd = np.diff(p)
    m = np.mod(dd + np.pi, 2.0 * np.pi) - np.pi
    m = np.where((m == -np.pi) & (dd > 0.0), np.pi, m)
    corr = np.where(np.abs(dd) < np.pi, 0.0, m - dd)
    un = p.copy()
    un[1:] = p[1:] + np.cumsum(corr)
    hs = box_mean(un * DEG, heading_window)
    v = np.empty(T)
    v[1:-1] = (hs[2:] - hs[:-2]) / 2.0
    v[0], v[-1] = hs[1] - hs[0], hs[-1] - hs[-2]
    vs = box_mean(v, velocity_window)
    extrema = np.nonzero(vs[:-1] * vs[1:] < 0.0)[0] + 1
    bounds = [0]
    while True:
        k = np.searchsorted(extrema, bounds[-1] + min_turn_frames)
        if k >= extrema.size:
            break
        bounds.append(int(extrema[k]))
    if T - 1 - bounds[-1] >= 1:
        bounds.append(T - 1)
    segments = [(s, e, float(hs[e] - hs[s])) for s, e in zip(bounds[:-1], bounds[1:])]
    kept = [(s, e, d) for s, e, d in segments if not e - s + 1 < min_turn_frames and not abs(d) < min_heading_change_deg]
    return hs, vs, kept, dict(dd=dd, extrema=extrema, segments=segments)


def turn_stats(all_series, kept, slots):
    """[42, T], kept turns -> stats [slots, 42, 4] (mean, population std, min, max over the finite samples), counts [slots, 42]"""
    S = all_series.shape[0]
    stats, counts = np.full((slots, S, 4), np.nan), np.zeros((slots, S), dtype=np.int32)
    for t, (s, e, _) in enumerate(kept):
        for k in range(S):
            x = all_series[k, s:e + 1]
            x = x[np.isfinite(x)]
            counts[t, k] = x.size
            if x.size:
                mean = np.mean(x)
                stats[t, k] = mean, np.sqrt(np.mean((x - mean) ** 2)), x.min(), x.max()
    return stats, counts


def kinematics(X, lengths=None, layout=MHR70_15, up_axis=(0.0, -1.0, 0.0), min_turn_frames=12, min_heading_change_deg=8.0,
               heading_window=11, velocity_window=9):
    """X [B, T, J, 3] or [T, J, 3] -> dict of arrays named and shaped as geometry.KinematicsResult's fields, plus "debug": one
    dict per clip with the quantities the discrete decisions hang on."""
    X = np.asarray(X, dtype=np.float64)
    if X.ndim == 3:
        X = X[None]
    B, T = X.shape[:2]
    M = max_turns(T, min_turn_frames)
    lengths = np.full(B, T) if lengths is None else np.clip(np.asarray(lengths, dtype=np.int64), 0, T)
    r = dict(series=np.full((B, 14, T), np.nan), changes=np.full((B, 28, T), np.nan), heading=np.full((B, T), np.nan),
             heading_smooth=np.full((B, T), np.nan), velocity_smooth=np.full((B, T), np.nan), boundary=np.zeros((B, T), dtype=bool),
             n_turns=np.zeros(B, dtype=np.int32), turn_frames=np.zeros((B, M, 2), dtype=np.int32),
             turn_heading_change=np.full((B, M), np.nan), turn_direction=np.zeros((B, M), dtype=np.int32),
             turn_stats=np.full((B, M, 42, 4), np.nan), turn_counts=np.zeros((B, M, 42), dtype=np.int32), debug=[])
    for b in range(B):
        n = int(lengths[b])
        s, h, dbg = base_series(X[b, :n], layout, up_axis)
        c = changes(s)
        hs, vs, kept, dbg2 = turns(h, min_turn_frames, min_heading_change_deg, heading_window, velocity_window)
        r["series"][b, :, :n], r["changes"][b, :, :n], r["heading"][b, :n] = s, c, h
        r["heading_smooth"][b, :n], r["velocity_smooth"][b, :n] = hs, vs
        r["n_turns"][b] = len(kept)
        for t, (st, en, d) in enumerate(kept):
            r["turn_frames"][b, t] = st, en
            r["turn_heading_change"][b, t] = d
            r["turn_direction"][b, t] = 1 if d > 0.0 else -1
            r["boundary"][b, [st, en]] = True
        r["turn_stats"][b], r["turn_counts"][b] = turn_stats(np.concatenate([s, c]), kept, M)
        r["debug"].append({**dbg, **dbg2, "velocity_smooth": vs, "kept": kept})
    return r
