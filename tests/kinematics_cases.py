"""Inputs of the kinematics tests: seeded synthetic skiers and the cases built from them.

skier() poses a 13-role skeleton (y down, x to the skier's right, z forward) with bent knees and elbows and a forward lean,
turns it about the vertical by a yaw that swings with a 60-frame period and 35 degrees around 170 (so the heading crosses
+-180), moves it downhill and adds a little seeded noise.  No limb is straight, the torso and the knees are well in front of
the pelvis, and the yaw's extrema are isolated: every discrete decision of the analysis has a margin
(tests/test_kinematics_cpu.py asserts them).  GOLDEN names the clips tools/make_goldens.py runs the reference on."""
import numpy as np

import kinematics_restated as kr

NAN = float("nan")


def yaw_swing(T, centre=170.0, amplitude=35.0, period=60.0, phase=0.0):
    return centre + amplitude * np.sin(2.0 * np.pi * (np.arange(T) + phase) / period)


def skier(T, seed, layout=kr.MHR70_15, joints=15, yaw=None, noise=0.002, y_up=False, move=True):
    """-> X [T, joints, 3] float64"""
    rng = np.random.default_rng(seed)
    t = np.arange(T, dtype=np.float64)
    yaw = yaw_swing(T) if yaw is None else np.broadcast_to(np.asarray(yaw, dtype=np.float64), (T,))
    lean = 0.35 + 0.10 * np.sin(2 * np.pi * t / 47.0)                 # torso forward lean (rad)
    z0, o = np.zeros(T), np.ones(T)
    P = {}
    neck = np.stack([z0, -0.5 * np.cos(lean), 0.5 * np.sin(lean)], axis=1)
    P["neck"] = neck
    for side, sx, ph in (("l", -1.0, 0.0), ("r", 1.0, 1.3)):
        hip = np.stack([sx * 0.12 * o, z0, z0], axis=1)
        beta = 0.75 + 0.20 * np.sin(2 * np.pi * t / 31.0 + ph)        # hip flexion
        gamma = 0.45 + 0.15 * np.sin(2 * np.pi * t / 23.0 + ph)       # shank back from the vertical
        knee = hip + 0.42 * np.stack([z0, np.cos(beta), np.sin(beta)], axis=1)
        foot = knee + 0.42 * np.stack([z0, np.cos(gamma), -np.sin(gamma)], axis=1)
        sho = neck + np.stack([sx * 0.18 * o, 0.03 * o, z0], axis=1)
        a = 0.5 + 0.2 * np.sin(2 * np.pi * t / 37.0 + ph)
        upper = np.stack([sx * 0.3 * o, 0.8 * o, a], axis=1)
        fore = np.stack([-sx * 0.2 * o, 0.2 + 0.2 * np.cos(2 * np.pi * t / 29.0 + ph), 0.95 * o], axis=1)
        elbow = sho + 0.28 * upper / np.linalg.norm(upper, axis=1, keepdims=True)
        hand = elbow + 0.25 * fore / np.linalg.norm(fore, axis=1, keepdims=True)
        for name, p in (("hip", hip), ("knee", knee), ("foot", foot), ("shoulder", sho), ("elbow", elbow), ("hand", hand)):
            P[f"{name}_{side}"] = p
    X = rng.normal(0.0, 0.3, size=(T, joints, 3))                     # the joints without a role: anything
    for role, j in zip(kr.ROLES, layout):
        if j >= 0:
            X[:, j] = P[role] + (rng.normal(0.0, noise, size=(T, 3)) if noise else 0.0)
    psi = np.radians(yaw)[:, None]
    x, z = X[..., 0].copy(), X[..., 2].copy()
    X[..., 0] = x * np.cos(psi) + z * np.sin(psi)
    X[..., 2] = -x * np.sin(psi) + z * np.cos(psi)
    if move:
        X = X + np.stack([0.02 * t, 0.01 * t, 0.05 * t], axis=1)[:, None, :]
    if y_up:
        X[..., 1] = -X[..., 1]
    return np.ascontiguousarray(X)


def _case(X, **kw):
    return dict(X=X, **kw)


def _golden_clips():
    hip_l, hip_r = kr.MHR70_15[4], kr.MHR70_15[5]
    g = {}
    g["g11"] = _case(skier(11, 101))
    X = skier(13, 102)
    X[[0, 12]] = NAN                                                  # whole frames missing at both ends
    g["g13"] = _case(X)
    X = skier(64, 103)
    X[20:30, hip_l] = NAN                                             # one hip missing: the shoulders give the heading
    X[40:43, hip_r, 1] = NAN
    g["g64"] = _case(X)
    g["g64_up"] = _case(skier(64, 104, y_up=True), up_axis=(0.0, 1.0, 0.0))
    X = skier(243, 105)
    X[:2] = NAN
    X[100:105] = NAN                                                  # whole frames missing in the middle
    X[241:] = NAN
    X[150:170, hip_l] = NAN
    X[60:64, 4] = NAN                                                 # an elbow
    X[200:203, 14, 2] = np.inf                                        # the neck
    X[106:136, 12] = NAN                                              # the right hand, for the whole of a turn
    g["g243"] = _case(X)
    return g


GOLDEN = _golden_clips()


def zero_limb_ties(X):
    """puts joints of the "zero_limb" case on one another, exactly"""
    X[5:9, kr.MHR70_15[8]] = X[5:9, kr.MHR70_15[6]]                   # foot_l on knee_l: a zero-length limb
    X[12:14, kr.MHR70_15[12]] = X[12:14, kr.MHR70_15[4]]              # neck on hip_l
    return X


def _more_cases():
    c = {}
    for T in (0, 1, 4, 5, 10, 11, 12, 13, 63, 64, 65, 1025, 4099):
        c[f"t{T}"] = _case(skier(T, 200 + T))
    T = 80
    clips = [skier(64, 103), skier(80, 301), skier(13, 302)]
    lengths = [64, 80, 13]
    X = np.empty((3, T, 15, 3))
    rng = np.random.default_rng(7)
    for b, (x, n) in enumerate(zip(clips, lengths)):
        X[b, :n] = x
        X[b, n:] = rng.choice([NAN, np.inf, -np.inf, 1e300, 0.0, 1.0], size=(T - n, 15, 3))
    c["ragged"] = _case(X, lengths=lengths)
    X = skier(40, 310)
    X[np.arange(40) != 17] = NAN
    c["one_heading"] = _case(X)
    X = skier(40, 311)
    X[:, [kr.MHR70_15[4], kr.MHR70_15[0]]] = NAN                      # left hip and left shoulder: no heading anywhere
    c["no_heading"] = _case(X)
    # heading exactly 0 in every frame: no yaw, no noise, no motion, so every velocity is exactly 0 (0 * 0 is no sign change)
    c["constant_heading"] = _case(skier(40, 312, yaw=0.0, noise=0.0, move=False))
    c["short_last"] = _case(skier(54, 313))                           # extrema near 15 and 46: the last segment has 8 frames
    amp = np.where(np.arange(130) < 60, 35.0, 3.0)
    c["small_change"] = _case(skier(130, 314, yaw=170.0 + amp * np.sin(2 * np.pi * np.arange(130) / 60.0)))
    c["zero_limb"] = _case(zero_limb_ties(skier(30, 315)))
    lay = list(kr.MHR70_15)
    lay[10], lay[12] = -1, -1                                         # no left hand, no neck
    c["absent_role"] = _case(skier(30, 316), layout=tuple(lay))
    c["h36m"] = _case(skier(70, 317, layout=kr.H36M_17, joints=17), layout=kr.H36M_17)
    c["params"] = _case(skier(90, 318), min_turn_frames=5, min_heading_change_deg=4.0, heading_window=5, velocity_window=3)
    return c


CASES = {**GOLDEN, **_more_cases()}

# the exactly straight limb, apart from CASES: the left knee is put on the midpoint of hip and foot in frames 3..5, so its
# cosine is -1 to a few ulps and the angle's error is that of acos at the end of its domain
STRAIGHT_FRAMES = (3, 4, 5)


def straight_case():
    X = skier(20, 320)
    hip, knee, foot = kr.MHR70_15[4], kr.MHR70_15[6], kr.MHR70_15[8]
    for t in STRAIGHT_FRAMES:
        X[t, knee] = (X[t, hip] + X[t, foot]) / 2.0
    return _case(X)


def params(case):
    """the keywords of kinematics() a case sets"""
    return {k: v for k, v in case.items() if k != "X"}


_restated = {}


def restated(name):
    """the restatement's result of a case, computed once and shared"""
    if name not in _restated:
        case = straight_case() if name == "straight" else CASES[name]
        _restated[name] = kr.kinematics(case["X"], **params(case))
    return _restated[name]


FLOAT_FIELDS = ("series", "changes", "heading", "heading_smooth", "velocity_smooth", "turn_heading_change", "turn_stats")
EXACT_FIELDS = ("boundary", "n_turns", "turn_frames", "turn_direction", "turn_counts")


def worst(got, want):
    """max |got - want| / (1 + |want|) after asserting equal shapes and NaN masks"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), "NaN masks differ"
    ok = ~np.isnan(want)
    if not ok.any():
        return 0.0
    assert np.array_equal(np.isinf(got[ok]), np.isinf(want[ok]))
    fin = ok & np.isfinite(want)
    return float(np.max(np.abs(got[fin] - want[fin]) / (1.0 + np.abs(want[fin])))) if fin.any() else 0.0
