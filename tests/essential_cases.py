"""Seeded inputs of the essential-matrix tests (tests/test_essential_{cpu,gpu}.py), built on resect_cases.rig: the 17-joint
skeleton 4-5 units away seen at f ~ 1100 px by two cameras, with pixel noise, gross outliers (keypoints moved by sigma =
80 px), detector scores, masking, and a view pair with different K of which one has skew.  The restatement's results are
computed once per case and shared (lru_cache); nothing changes them."""
import functools

import numpy as np

import essential_restated as er
import resect_cases as rc
from resect_restated import normalised_rays

J = rc.J
MIN_CONF = 0.5
N_SOLVER_SAMPLES = 500


def pair(c, v0=0, v1=1):
    """views (v0, v1) of a rig as a two-view problem: x2d [2,N,2], K [2,3,3], conf [2,N] | None, the true R_rel, t_rel"""
    x2d = np.stack([c["x2d"][v0].reshape(-1, 2), c["x2d"][v1].reshape(-1, 2)])
    K = np.stack([c["K"][v0], c["K"][v1]])
    conf = None if c["conf"] is None else np.stack([c["conf"][v0].reshape(-1), c["conf"][v1].reshape(-1)])
    R = c["R"][v1] @ c["R"][v0].T
    t = c["t"][v1] - R @ c["t"][v0]
    return dict(x2d=x2d, K=K, conf=conf, R=R, t=t / np.linalg.norm(t), T=c["T"])


# name -> (rig arguments, views, per-frame groups, keywords of essential_ransac).  The RANSAC seeds are those at which
# test_essential_cpu.test_comparison_case_is_stable holds (a subset of 17 points drawn twice ties with itself to rounding);
# seeds that differ only below the bits of the hypothesis index give the same samples in another order (rule 3's XOR)
_TABLE = [
    ("clean_T1", dict(T=1, V=2, seed=41), (0, 1), False, dict(hypotheses=64, seed=1)),
    ("clean_T8_step", dict(T=8, V=2, seed=42), (0, 1), True, dict(hypotheses=64, seed=2)),
    ("clean_T64_clip", dict(T=64, V=2, seed=43), (0, 1), False, dict(hypotheses=64, seed=3)),
    ("clean_T64_clip_skewK", dict(T=64, V=3, seed=44), (0, 2), False, dict(hypotheses=64, seed=4)),
    ("noise1_T1", dict(T=1, V=2, seed=45, noise=1.0), (0, 1), False, dict(hypotheses=256, seed=4101)),
    ("noise1_T8_step", dict(T=8, V=2, seed=46, noise=1.0), (0, 1), True, dict(hypotheses=256, seed=4102)),
    ("noise1_T64_clip", dict(T=64, V=2, seed=47, noise=1.0), (0, 1), False, dict(hypotheses=256, seed=4103)),
    ("noise1_T64_clip_skewK", dict(T=64, V=3, seed=48, noise=1.0), (0, 2), False, dict(hypotheses=256, seed=4104)),
    ("out10_T64_clip", dict(T=64, V=2, seed=49, noise=1.0, outliers=0.10), (0, 1), False, dict(hypotheses=300, seed=9)),
    ("out30_T64_clip", dict(T=64, V=2, seed=50, noise=1.0, outliers=0.30), (0, 1), False, dict(hypotheses=512, seed=4106)),
    ("out10_T8_step", dict(T=8, V=2, seed=51, noise=1.0, outliers=0.10), (0, 1), True, dict(hypotheses=256, seed=4107)),
    ("out10_T1", dict(T=1, V=2, seed=52, noise=1.0, outliers=0.10), (0, 1), False, dict(hypotheses=256, seed=4108)),
    ("conf_T8_step", dict(T=8, V=2, seed=53, noise=1.0, with_conf=True), (0, 1), True,
     dict(hypotheses=256, seed=16397, min_conf=MIN_CONF)),
    ("conf_T64_clip", dict(T=64, V=2, seed=54, noise=1.0, outliers=0.10, with_conf=True), (0, 1), False,
     dict(hypotheses=256, seed=4110, min_conf=MIN_CONF)),
]


@functools.lru_cache(maxsize=None)
def cases():
    """-> tuple of (name, two-view problem, keywords of essential_ransac without x2d / K / conf)"""
    out = []
    for name, args, views, per_step, kw in _TABLE:
        p = pair(rc.rig(**args), *views)
        out.append((name, p, dict(kw, group_size=J if per_step else None)))
    return tuple(out)


def clean_cases():
    return [c for c in cases() if c[0].startswith("clean")]


def comparison_cases():
    """the cases compared through `winner` and the floats: every one but the noise-free ones, whose costs are rounding"""
    return [c for c in cases() if not c[0].startswith("clean")]


def case(name):
    return next(c for c in cases() if c[0] == name)


MASKED_FAILED, MASKED_FIVE = 2, 5


@functools.lru_cache(maxsize=None)
def masked_case():
    """T = 8 frames as per-frame groups, with scores and min_conf: group 2 keeps 4 points and fails (5 with a NaN keypoint
    in view 0, 4 in view 1 only, 4 with a score of view 0 under min_conf); group 5 keeps exactly 5; groups 0, 4 and 6 lose
    one point each to one of the three causes; non-finite and out-of-range scores elsewhere exercise the clipping."""
    c = rc.rig(T=8, V=2, seed=61, noise=1.0, with_conf=True)
    x2d, conf = c["x2d"].copy(), np.clip(c["conf"] + 0.2, 0.0, 1.0)      # scores in [0.6, 1]: only what follows masks
    x2d[0, 2, 0:5, 1] = np.nan
    x2d[1, 2, 5:9, 0] = np.inf
    conf[0, 2, 9:13] = 0.1
    x2d[0, 5, 0:4, 0] = np.nan
    x2d[1, 5, 4:8, 1] = np.nan
    conf[1, 5, 8:12] = 0.3
    x2d[0, 0, 3, 0] = np.nan
    x2d[1, 4, 5, 1] = -np.inf
    conf[1, 6, 7] = 0.49
    conf[0, 1, 2] = 1.7          # clipped to 1
    conf[1, 3, 9] = np.nan       # -> 0 < min_conf: masked
    conf[0, 7, 0] = -np.inf      # -> 0: masked
    p = pair(dict(c, x2d=x2d, conf=conf))
    n_used = np.array([16, 17, 4, 16, 16, 5, 16, 16])
    return "masked_T8_step", p, dict(hypotheses=256, seed=8213, min_conf=MIN_CONF, group_size=J), n_used


@functools.lru_cache(maxsize=None)
def restated(name):
    """the restatement's result of a case, with the details the stability conditions need"""
    _, p, kw = masked_case()[:3] if name == "masked_T8_step" else case(name)
    return er.essential_ransac(p["x2d"], p["K"], conf=p["conf"], details=True, **kw)


@functools.lru_cache(maxsize=None)
def solver_samples():
    """N_SOLVER_SAMPLES five-point samples (a, b [S,5,2] normalised) from three rigs: noise-free, 1 px, 1 px with outliers"""
    a, b = [], []
    for seed, noise, outliers, n in ((71, 0.0, 0.0, 200), (72, 1.0, 0.0, 150), (73, 1.0, 0.1, 150)):
        p = pair(rc.rig(T=64, V=3, seed=seed, noise=noise, outliers=outliers), 0, 2)
        ua = np.stack(normalised_rays(p["K"][0], p["x2d"][0]), axis=1)
        ub = np.stack(normalised_rays(p["K"][1], p["x2d"][1]), axis=1)
        rng = np.random.default_rng(seed)
        idx = np.array([rng.choice(ua.shape[0], 5, replace=False) for _ in range(n)])
        a.append(ua[idx])
        b.append(ub[idx])
    return np.concatenate(a), np.concatenate(b)


@functools.lru_cache(maxsize=None)
def solver_restated():
    a, b = solver_samples()
    return er.five_point(a, b, details=True)


def rotation_angle_deg(R, R_true):
    c = (np.trace(R @ R_true.T) - 1.0) / 2.0
    return float(np.degrees(np.arccos(np.clip(c, -1.0, 1.0))))


def direction_angle_deg(t, t_true):
    c = float(t @ t_true) / (np.linalg.norm(t) * np.linalg.norm(t_true))
    return float(np.degrees(np.arccos(np.clip(c, -1.0, 1.0))))
