"""Inputs of the evaluation tests: seeded float64 (prediction, target) clips and the cases built from them.

pose_clip() moves a seeded skeleton whose extent differs along the three axes (so the singular values of the Procrustes
problem are well apart) smoothly through time; the prediction is that clip under a small rotation, a scale, an offset and
seeded noise.  The cases cover every frame count at which the code takes another path (0, 1, 2: no velocity or second
difference; 3, 4: the smallest percentile problems and an odd and an even median; 21 at J = 17 and 41 at J = 15: integer and
fractional percentile ranks; 300: past one workgroup's width), J in {1, 15, 17, 70} (one lane, one wave, two joints per
lane), missing joints in all the ways the rules name, a mirrored frame (det R < 0), a frame without extent, zero_root on and
off, and a ragged batch with garbage beyond each length.  The clip under quality assessment is the prediction.
ASSERTED at import: every complete frame's H has its two smallest singular values at least 1e-3 apart; otherwise the
reflection fix is ill-conditioned and no tolerance means anything."""
import numpy as np

import evaluate_restated as er

NAN = float("nan")
MHR70_15_EDGES = ((14, 2), (2, 4), (4, 13), (14, 3), (3, 5), (5, 12), (14, 6), (6, 8), (8, 10), (14, 7), (7, 9), (9, 11), (6, 7), (2, 3))
MHR70_15_LEFT_BONES = ((14, 2), (2, 4), (4, 13), (14, 6), (6, 8), (8, 10))
MHR70_15_RIGHT_BONES = ((14, 3), (3, 5), (5, 12), (14, 7), (7, 9), (9, 11))
MHR70_15_LR_PAIRS = ((0, 1), (2, 3), (4, 5), (6, 7), (8, 9), (10, 11), (13, 12))
MIN_SV_GAP = 1e-3


def layout(J):
    """the index lists of clip_quality for a clip of J joints"""
    if J == 17:
        return dict(edges=er.H36M_EDGES, left_edges=er.H36M_LEFT_BONES, right_edges=er.H36M_RIGHT_BONES, lr_pairs=er.H36M_LR_PAIRS)
    if J == 15:
        return dict(edges=MHR70_15_EDGES, left_edges=MHR70_15_LEFT_BONES, right_edges=MHR70_15_RIGHT_BONES, lr_pairs=MHR70_15_LR_PAIRS)
    if J == 1:
        return dict(edges=(), left_edges=(), right_edges=(), lr_pairs=((0, 0),))
    chain = tuple((j, j + 1) for j in range(J - 1))                  # 69 edges at J = 70
    return dict(edges=chain, left_edges=chain[0::2], right_edges=chain[1::2], lr_pairs=tuple((j, J - 1 - j) for j in range(J // 2)))


def _rot(axis, angle):
    axis = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def pose_clip(T, J, seed, noise=0.02):
    """-> pred, target [T, J, 3] float64"""
    rng = np.random.default_rng(seed)
    t = np.arange(T, dtype=np.float64)[:, None, None]
    base = rng.normal(0.0, 1.0, size=(J, 3)) * np.array([0.25, 0.6, 0.15])
    phase, amp = rng.uniform(0, 2 * np.pi, size=(J, 3)), rng.uniform(0.02, 0.08, size=(J, 3))
    target = base[None] + amp[None] * np.sin(2 * np.pi * t / 23.0 + phase[None]) + np.array([0.03, 0.01, 0.05]) * t
    pred = 1.05 * target @ _rot(rng.normal(size=3), 0.1).T + rng.normal(0.0, noise, size=(T, J, 3)) + np.array([0.1, -0.05, 0.2])
    return np.ascontiguousarray(pred), np.ascontiguousarray(target)


def _case(pred, target, **kw):
    return dict(pred=pred, target=target, **kw)


def _clean(T, J, seed, **kw):
    return _case(*pose_clip(T, J, seed), **kw)


def _missing():
    """T = 21, J = 17: everything the rules name, and with it a percentile that is NaN (joint 3 has no finite sample)"""
    p, g = pose_clip(21, 17, 101)
    p[5] = NAN                              # a whole frame
    p[:, 3] = NAN                           # a joint missing for the whole clip: n = 0, a series without a finite sample
    g[:, 4, 1] = NAN
    g[9, 4, 1] = 0.3                        # a series with exactly one finite sample (the target's; the joint is valid once)
    p[:3, 6] = NAN                          # a leading run
    p[18:, 7] = NAN                         # a trailing run
    p[8:12, 8, 2] = NAN                     # a gap in one coordinate
    p[14, 10, 0] = np.inf                   # an infinite coordinate is as missing as a NaN
    g[2, 12] = NAN                          # missing in the target only
    p[:, 13, 2] = NAN
    p[9, 13, 2] = 0.3                       # the same in the clip under quality assessment: np.interp leaves it alone
    return _case(p, g)


def _gaps():
    """T = 41, J = 15: runs at both ends and inside, every series keeps at least 2 finite samples: finite percentiles"""
    p, g = pose_clip(41, 15, 102)
    p[:4, 2] = NAN
    p[37:, 5] = NAN
    p[10:19, 8, 0] = NAN
    p[20, 9] = NAN
    p[22, 9] = NAN
    p[1:40, 11, 1] = NAN                    # exactly 2 finite samples, the ends
    g[30:33, 14] = NAN
    return _case(p, g)


def _mirror():
    """T = 4, J = 17: frame 2 of the prediction is the target mirrored in x, so det R < 0 before the fix"""
    p, g = pose_clip(4, 17, 103)
    p[2] = g[2] * np.array([-1.0, 1.0, 1.0]) + np.random.default_rng(7).normal(0.0, 0.01, size=(17, 3))
    return _case(p, g)


def _flat():
    """T = 4, J = 17: frame 1 of the prediction has all joints at one point (dyadic, so its mean is exact in any order)"""
    p, g = pose_clip(4, 17, 104)
    p[1] = np.array([0.5, -0.25, 1.0])
    return _case(p, g)


def _ragged():
    """3 clips, T = 41, J = 17, lengths 41, 18, 0 with NaN / inf / huge garbage beyond each length"""
    rng = np.random.default_rng(105)
    P, G = np.empty((3, 41, 17, 3)), np.empty((3, 41, 17, 3))
    lens = (41, 18, 0)
    for b, n in enumerate(lens):
        P[b], G[b] = pose_clip(41, 17, 200 + b)
        for A in (P, G):
            junk = rng.choice(np.array([NAN, np.inf, -np.inf, 1e300, 0.0]), size=(41 - n, 17, 3))
            A[b, n:] = junk
    P[1, 3:6, 4] = NAN
    P[1, 17, 9] = NAN
    G[0, 11] = NAN
    return _case(P, G, lengths=lens)


CASES = {}
for _T in (0, 1, 2, 3, 4, 21, 41, 300):
    CASES[f"clean_T{_T}_J17"] = _clean(_T, 17, 10 + _T)
CASES["clean_T41_J15"] = _clean(41, 15, 61)
CASES["clean_T4_J15"] = _clean(4, 15, 62)
CASES["clean_T3_J1"] = _clean(3, 1, 63)
CASES["clean_T21_J1"] = _clean(21, 1, 64)
CASES["clean_T4_J70"] = _clean(4, 70, 65)
CASES["clean_T21_J70"] = _clean(21, 70, 66)
CASES["zero_root_T21_J17"] = _clean(21, 17, 67, zero_root=0)
CASES["zero_root_T4_J15"] = _clean(4, 15, 68, zero_root=14)
CASES["missing_T21_J17"] = _missing()
CASES["missing_zero_root_T21_J17"] = dict(_missing(), zero_root=12)      # the target's missing joint 12 counts as the origin
CASES["gaps_T41_J15"] = _gaps()
CASES["mirror_T4_J17"] = _mirror()
CASES["flat_T4_J17"] = _flat()
CASES["ragged_B3_T41_J17"] = _ragged()

# the NaN-free single clips tools/make_goldens.py runs loss.py's p_mpjpe on (it raises or returns NaN otherwise)
NAN_FREE = tuple(k for k, c in CASES.items() if c["pred"].ndim == 3 and c["pred"].shape[0] >= 1 and c["pred"].shape[1] > 1 and
                 np.isfinite(c["pred"]).all() and np.isfinite(c["target"]).all() and not k.startswith("flat"))
# evaluate_clips' clips: lists of NaN-free clips of different lengths
EVAL_CLIPS = {"h36m": ("clean_T21_J17", "clean_T41_J17", "clean_T4_J17", "mirror_T4_J17", "clean_T2_J17"), "mhr": ("clean_T41_J15", "clean_T4_J15")}
# eval_fused_pose's (left, right, fused): the fused clip is the mean of the finite ones of two views
FUSED = ("clean_T21_J17", "clean_T2_J17", "clean_T300_J17", "missing_T21_J17")


def fused_inputs(name):
    c = CASES[name]
    left, right = c["pred"], c["target"]
    with np.errstate(all="ignore"):
        both = np.isfinite(left).all(axis=2, keepdims=True) & np.isfinite(right).all(axis=2, keepdims=True)
        fused = np.where(both, 0.5 * (left + right), np.where(np.isfinite(left).all(axis=2, keepdims=True), left, right))
    return left, right, np.ascontiguousarray(fused)


def params(case):
    return {k: case[k] for k in ("lengths", "zero_root") if k in case}


def clips_of(case):
    """-> [(pred [n, J, 3], target [n, J, 3])] of the case's clips cut to their lengths"""
    P, G = case["pred"], case["target"]
    if P.ndim == 3:
        return [(P, G)]
    return [(P[b, :n], G[b, :n]) for b, n in enumerate(case["lengths"])]


_restated = {}


def restated(name):
    """the restatement's outputs of a case, computed once: (pose_errors dict, clip_quality dict)"""
    if name not in _restated:
        c = CASES[name]
        J = c["pred"].shape[-2]
        _restated[name] = (er.pose_errors(c["pred"], c["target"], **params(c)),
                           er.clip_quality(c["pred"], lengths=c.get("lengths"), **layout(J)))
    return _restated[name]


def sv_gaps():
    """name -> the smallest gap between the two smallest singular values of H over the case's complete frames"""
    out = {}
    for name, c in CASES.items():
        zr = c.get("zero_root")
        worst = np.inf
        for p, g in clips_of(c):
            g = g.copy()
            if zr is not None:
                g[:, zr] = 0.0
            with np.errstate(all="ignore"):
                full = np.isfinite(p).all(axis=(1, 2)) & np.isfinite(g).all(axis=(1, 2))
                if p.shape[1] > 1 and full.any():
                    s = er.singular_values(p[full], g[full])
                    if s.size:
                        worst = min(worst, float((s[:, 1] - s[:, 2]).min()))
        out[name] = worst
    return out


SV_GAPS = sv_gaps()
assert all(v >= MIN_SV_GAP for v in SV_GAPS.values()), {k: v for k, v in SV_GAPS.items() if v < MIN_SV_GAP}
