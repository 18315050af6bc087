"""Seeded inputs of the camera-and-points refinement tests (tests/test_refine_{cpu,gpu}.py), built like
tests/resect_cases.py: a random-walk 17-joint skeleton seen by one to four cameras about 6 m away with K ~ 1100 px, 1 px
keypoint noise, and the lifter's joints X0 = truth plus 5 cm noise (DESIGN §2 "Camera + points refinement")."""
import numpy as np

from resect_cases import F_SCALE, MIN_CONF, look_at, start_near_truth   # noqa: F401

J = 17


def rig(T, V, seed, noise=1.0, x_noise=0.05, outliers=0.0, with_conf=False, joints=J):
    """-> dict: Xtrue, X [T,joints,3] (X = Xtrue + x_noise N(0,1)), x2d, clean [V,T,joints,2], moved [V,T,joints],
    K [V,3,3], R [V,3,3], t [V,3], conf [V,T,joints] | None"""
    rng = np.random.default_rng(seed)
    base = rng.uniform(-0.5, 0.5, (joints, 3)) * np.array([0.8, 0.6, 1.8])
    walk = np.cumsum(rng.normal(0, 0.02, (T, 1, 3)), axis=0) + np.cumsum(rng.normal(0, 0.01, (T, joints, 3)), axis=0)
    Xt = base[None] + walk
    K, R, t = np.zeros((V, 3, 3)), np.zeros((V, 3, 3)), np.zeros((V, 3))
    for v in range(V):
        az = 2 * np.pi * v / 5 + rng.uniform(-0.2, 0.2)
        d = rng.uniform(5.5, 6.5)
        C = Xt.mean(axis=(0, 1)) + d * np.array([np.cos(az) * 0.95, np.sin(az) * 0.95, rng.uniform(0.1, 0.3)])
        R[v] = look_at(C, Xt.mean(axis=(0, 1)) + rng.normal(0, 0.05, 3))
        t[v] = -R[v] @ C
        K[v] = [[1100 + rng.uniform(-20, 20), 0.5 if v == 2 else 0.0, 960 + rng.uniform(-5, 5)],
                [0, 1100 + rng.uniform(-20, 20), 540 + rng.uniform(-5, 5)], [0, 0, 1]]
    Xc = np.einsum("vab,tjb->vtja", R, Xt) + t[:, None, None, :]
    u, w = Xc[..., 0] / Xc[..., 2], Xc[..., 1] / Xc[..., 2]
    clean = np.stack([K[:, 0, 0, None, None] * u + K[:, 0, 1, None, None] * w + K[:, 0, 2, None, None],
                      K[:, 1, 1, None, None] * w + K[:, 1, 2, None, None]], axis=-1)
    x2d = clean + noise * rng.normal(0, 1, clean.shape)
    moved = rng.uniform(0, 1, (V, T, joints)) < outliers
    x2d = x2d + moved[..., None] * rng.normal(0, 80.0, clean.shape)
    conf = rng.uniform(0.4, 1.0, (V, T, joints)) if with_conf else None
    X = Xt + x_noise * rng.normal(0, 1, Xt.shape)
    return dict(Xtrue=Xt, X=X, x2d=x2d, clean=clean, moved=moved, K=K, R=R, t=t, conf=conf, T=T, V=V, J=joints)


def flat(c):
    """the (N, .) arrays of a rig: X [N,3], x2d [V,N,2], conf [V,N] | None"""
    V = c["V"]
    return c["X"].reshape(-1, 3), c["x2d"].reshape(V, -1, 2), None if c["conf"] is None else c["conf"].reshape(V, -1)


def start(c, per_step, seed=100, angle=0.01, shift=0.03):
    """R0 [G,V,3,3], t0 [G,V,3] near the true cameras (a given start, so that a case does not depend on the resection)"""
    return start_near_truth(c, c["T"] if per_step else 1, seed + c["T"] + 7 * c["V"], angle, shift)


# name -> (rig arguments, per-step grouping, K given, lambda_x, loss)
_TABLE = [
    ("n6_V2_lx1", dict(T=1, V=2, seed=41, joints=6), False, True, 1.0, "linear"),
    ("n6_V2_lx0", dict(T=1, V=2, seed=41, joints=6), False, True, 0.0, "linear"),
    ("step_V2_lx1", dict(T=5, V=2, seed=42), True, True, 1.0, "linear"),
    ("step_V2_lx100_soft", dict(T=5, V=2, seed=43, with_conf=True), True, True, 100.0, "soft_l1"),
    ("step_V2_lx0", dict(T=5, V=2, seed=42), True, True, 0.0, "linear"),
    ("step_V2_lx0_soft", dict(T=5, V=2, seed=44), True, True, 0.0, "soft_l1"),
    ("step_V3_lx1", dict(T=5, V=3, seed=45), True, True, 1.0, "linear"),
    ("step_V3_lx0_conf", dict(T=5, V=3, seed=46, with_conf=True), True, True, 0.0, "linear"),
    ("step_V4_lx100_soft", dict(T=5, V=4, seed=47), True, True, 100.0, "soft_l1"),
    ("step_V4_lx100_inferK", dict(T=5, V=4, seed=48), True, False, 100.0, "linear"),
    ("step_V1_lx1", dict(T=5, V=1, seed=49), True, True, 1.0, "linear"),
    ("step_V1_lx0", dict(T=5, V=1, seed=49), True, True, 0.0, "linear"),
    ("n65_V2_lx1", dict(T=1, V=2, seed=50, joints=65), False, True, 1.0, "linear"),
    ("n65_V3_lx0_soft", dict(T=1, V=3, seed=51, joints=65), False, True, 0.0, "soft_l1"),
    ("n1100_V2_lx100", dict(T=100, V=2, seed=52, joints=11), False, True, 100.0, "linear"),
    ("n1100_V2_lx0", dict(T=100, V=2, seed=52, joints=11), False, True, 0.0, "linear"),
]


def cases():
    """-> list of (name, rig, kwargs of refine_cameras_points without X / x2d / conf)"""
    out = []
    for name, args, per_step, k_given, lambda_x, loss in _TABLE:
        c = rig(**args)
        R0, t0 = start(c, per_step)
        out.append((name, c, dict(group_size=c["J"] if per_step else None, K=c["K"] if k_given else None, R0=R0, t0=t0,
                                  lambda_x=lambda_x, loss=loss, f_scale=F_SCALE if loss == "soft_l1" else 1.0)))
    return out


def prior_cases():
    return [x for x in cases() if x[2]["lambda_x"] > 0]


def masked_case():
    """T = 6 steps, per step, with scores and min_conf: group 2 keeps 5 points; groups 0, 3 and 4 lose one point each, to a
    NaN in X, a NaN keypoint in one view and a score under min_conf in one view"""
    c = rig(T=6, V=2, seed=61, with_conf=True)
    X, x2d, conf = c["X"].copy(), c["x2d"].copy(), c["conf"].copy()
    X[2, 0:4, 1] = np.nan
    x2d[1, 2, 4:8, 0] = np.nan
    conf[0, 2, 8:12] = 0.1
    X[0, 3, 2] = np.inf
    x2d[0, 3, 5, 1] = np.nan
    conf[1, 4, 7] = 0.29
    conf[0, 1, 2] = 1.7          # clipped to 1
    c = dict(c, X=X, x2d=x2d, conf=conf)
    R0, t0 = start(c, True)
    n_points = np.array([16, 17, 5, 16, 16, 17])
    masked = [(0, 3), (3, 5), (4, 7)]             # (step, joint) of the single masked points
    return ("masked_T6_V2_step", c, dict(group_size=J, K=c["K"], R0=R0, t0=t0, lambda_x=1.0, loss="linear", min_conf=MIN_CONF),
            n_points, masked)


def clip_outlier_case(seed):
    """the whole-clip case of check (g): T = 243 steps, 10 % keypoints moved by sigma = 80 px"""
    c = rig(T=243, V=2, seed=seed, outliers=0.10)
    R0, t0 = start(c, False)
    return c, dict(group_size=None, K=c["K"], R0=R0, t0=t0)


def pose_distance(R, t, R_true, t_true):
    """||R - R*||_F + ||t - t*||"""
    return np.sqrt(((R - R_true) ** 2).sum(axis=(-2, -1))) + np.sqrt(((t - t_true) ** 2).sum(axis=-1))


def true_relative(c):
    R_rel = c["R"][1] @ c["R"][0].T
    return R_rel, c["t"][1] - R_rel @ c["t"][0]
