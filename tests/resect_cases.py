"""Seeded inputs of the resection tests (tests/test_resect_{cpu,gpu}.py): a random-walk 17-joint skeleton seen by two or
three cameras 4-5 units away with K ~ 1100 px, pixel noise, gross outliers (keypoints moved by sigma = 80 px), detector
scores, and the masking inputs of rule 1 (DESIGN §2 "Resection")."""
import numpy as np

J = 17
F_SCALE = 2.0          # soft_l1 scale of the outlier cases: --huber 2 (f_scale = max(huber, 1), slove_rt_from_3d.py:244)
MIN_CONF = 0.3


def look_at(C, target):
    """world -> camera rotation of a camera at C looking at `target`, y down"""
    z = target - C
    z = z / np.linalg.norm(z)
    x = np.cross(z, np.array([0.0, 0.0, 1.0]))
    x = x / np.linalg.norm(x)
    y = np.cross(z, x)
    return np.stack([x, y, z])


def rig(T, V, seed, noise=0.0, outliers=0.0, with_conf=False):
    """-> dict: X [T,J,3], x2d [V,T,J,2], clean [V,T,J,2], moved [V,T,J], K [V,3,3], R [V,3,3], t [V,3], conf [V,T,J] | None"""
    rng = np.random.default_rng(seed)
    base = rng.uniform(-0.5, 0.5, (J, 3)) * np.array([0.8, 0.6, 1.8])
    walk = np.cumsum(rng.normal(0, 0.02, (T, 1, 3)), axis=0) + np.cumsum(rng.normal(0, 0.01, (T, J, 3)), axis=0)
    X = base[None] + walk
    K, R, t = np.zeros((V, 3, 3)), np.zeros((V, 3, 3)), np.zeros((V, 3))
    for v in range(V):
        az = 2 * np.pi * v / 3 + rng.uniform(-0.3, 0.3)
        d = rng.uniform(4.0, 5.0)
        C = X.mean(axis=(0, 1)) + d * np.array([np.cos(az) * 0.95, np.sin(az) * 0.95, rng.uniform(0.1, 0.3)])
        R[v] = look_at(C, X.mean(axis=(0, 1)) + rng.normal(0, 0.05, 3))
        t[v] = -R[v] @ C
        K[v] = [[1100 + rng.uniform(-20, 20), 0.5 if v == 2 else 0.0, 960 + rng.uniform(-5, 5)],
                [0, 1100 + rng.uniform(-20, 20), 540 + rng.uniform(-5, 5)], [0, 0, 1]]
    Xc = np.einsum("vab,tjb->vtja", R, X) + t[:, None, None, :]
    u, w = Xc[..., 0] / Xc[..., 2], Xc[..., 1] / Xc[..., 2]
    clean = np.stack([K[:, 0, 0, None, None] * u + K[:, 0, 1, None, None] * w + K[:, 0, 2, None, None],
                      K[:, 1, 1, None, None] * w + K[:, 1, 2, None, None]], axis=-1)
    x2d = clean + noise * rng.normal(0, 1, clean.shape)
    moved = rng.uniform(0, 1, (V, T, J)) < outliers
    x2d = x2d + moved[..., None] * rng.normal(0, 80.0, clean.shape)
    conf = rng.uniform(0.4, 1.0, (V, T, J)) if with_conf else None
    return dict(X=X, x2d=x2d, clean=clean, moved=moved, K=K, R=R, t=t, conf=conf, T=T, V=V)


def flat(c):
    """the (N, .) arrays of a rig: X [N,3], x2d [V,N,2], conf [V,N] | None"""
    V = c["V"]
    return c["X"].reshape(-1, 3), c["x2d"].reshape(V, -1, 2), None if c["conf"] is None else c["conf"].reshape(V, -1)


def sample_groups(G, seed, n=24):
    if G <= n:
        return list(range(G))
    return sorted(np.random.default_rng(seed).choice(G, n, replace=False).tolist())


# name -> (rig arguments, per-step grouping, K given)
_TABLE = [
    ("clean_T1_V2", dict(T=1, V=2, seed=1), False, True),
    ("clean_T64_V3_step", dict(T=64, V=3, seed=2), True, True),
    ("clean_T64_V2_clip", dict(T=64, V=2, seed=3), False, True),
    ("clean_T1024_V2_clip", dict(T=1024, V=2, seed=4), False, True),
    ("clean_T1024_V3_step", dict(T=1024, V=3, seed=5), True, True),
    ("noise1_T64_V2_step_conf", dict(T=64, V=2, seed=6, noise=1.0, with_conf=True), True, True),
    ("noise2_T64_V3_clip", dict(T=64, V=3, seed=7, noise=2.0), False, True),
    ("noise1_T1024_V2_step", dict(T=1024, V=2, seed=8, noise=1.0), True, True),
    ("noise1_T1_V3_conf", dict(T=1, V=3, seed=9, noise=1.0, with_conf=True), False, True),
    ("out5_T64_V2_clip", dict(T=64, V=2, seed=10, noise=1.0, outliers=0.05), False, True),
    ("out10_T64_V3_clip_conf", dict(T=64, V=3, seed=11, noise=2.0, outliers=0.10, with_conf=True), False, True),
    ("out10_T1024_V2_clip", dict(T=1024, V=2, seed=12, noise=1.0, outliers=0.10), False, True),
    ("out5_T1024_V2_clip", dict(T=1024, V=2, seed=13, noise=2.0, outliers=0.05), False, True),
    ("out10_T64_V2_step", dict(T=64, V=2, seed=14, noise=1.0, outliers=0.10), True, True),
    ("inferK_T64_V2_clip", dict(T=64, V=2, seed=15, noise=1.0), False, False),
    ("inferK_T64_V3_step_conf", dict(T=64, V=3, seed=16, noise=1.0, with_conf=True), True, False),
]


def cases():
    """-> list of (name, rig, kwargs of resect_cameras without X / x2d / conf, groups to compare)"""
    out = []
    for name, args, per_step, k_given in _TABLE:
        c = rig(**args)
        kw = dict(group_size=J if per_step else None, K=c["K"] if k_given else None)
        G = c["T"] if per_step else 1
        groups = sample_groups(G, args["seed"])
        if args.get("outliers", 0.0) > 0:
            out.append((name + "_linear", c, dict(kw, loss="linear"), groups))
            out.append((name + "_soft_l1", c, dict(kw, loss="soft_l1", f_scale=F_SCALE), groups))
        else:
            out.append((name, c, dict(kw, loss="linear"), groups))
    return out


def clean_cases():
    return [x for x in cases() if x[0].startswith("clean")]


def outlier_pairs():
    """-> list of (name, rig, kwargs linear, kwargs soft_l1, groups)"""
    cs = cases()
    lin = {n[:-7]: (c, kw, g) for n, c, kw, g in cs if n.endswith("_linear")}
    return [(n[:-8], c, lin[n[:-8]][1], kw, g) for n, c, kw, g in cs if n.endswith("_soft_l1")]


def start_near_truth(c, G, seed, angle=0.03, shift=0.1):
    """R0 [G,V,3,3], t0 [G,V,3]: the true pose turned by ~`angle` rad and moved by ~`shift`"""
    rng = np.random.default_rng(seed)
    V = c["V"]
    R0, t0 = np.zeros((G, V, 3, 3)), np.zeros((G, V, 3))
    for g in range(G):
        for v in range(V):
            w = rng.normal(0, angle, 3)
            th = np.linalg.norm(w)
            Kx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
            E = np.eye(3) + np.sin(th) / th * Kx + (1 - np.cos(th)) / th ** 2 * (Kx @ Kx)
            R0[g, v] = E @ c["R"][v]
            t0[g, v] = c["t"][v] + rng.normal(0, shift, 3)
    return R0, t0


def given_start_case():
    c = rig(T=64, V=2, seed=21, noise=1.0)
    R0, t0 = start_near_truth(c, 64, 22)
    return "given_R0_T64_V2_step", c, dict(group_size=J, K=c["K"], R0=R0, t0=t0, loss="linear"), list(range(0, 64, 4))


def masked_case():
    """T = 8 steps, per step, with scores and min_conf: group 2 keeps 5 points (4 joints NaN in X, 4 with a NaN keypoint in
    view 1 only, 4 with a score of view 0 under min_conf); groups 0, 4 and 6 lose one point each to one of the three causes;
    non-finite and out-of-range scores elsewhere exercise the clipping."""
    c = rig(T=8, V=2, seed=31, noise=1.0, with_conf=True)
    X, x2d, conf = c["X"].copy(), c["x2d"].copy(), c["conf"].copy()
    X[2, 0:4, 1] = np.nan
    x2d[1, 2, 4:8, 0] = np.nan
    conf[0, 2, 8:12] = 0.1
    X[0, 3, 2] = np.inf
    x2d[0, 4, 5, 1] = np.nan
    conf[1, 6, 7] = 0.29
    conf[0, 1, 2] = 1.7          # clipped to 1
    conf[1, 3, 9] = np.nan       # -> 0 < min_conf: masked
    conf[0, 5, 0] = -np.inf      # -> 0: masked
    c = dict(c, X=X, x2d=x2d, conf=conf)
    n_points = np.array([16, 17, 5, 16, 16, 16, 16, 17])
    return "masked_T8_V2_step", c, dict(group_size=J, K=c["K"], loss="linear", min_conf=MIN_CONF), list(range(8)), n_points


def removed(c, keep):
    """the rig with only the points keep [T*J] (bool), flattened: X [n,3], x2d [V,n,2], conf [V,n]"""
    X, x2d, conf = flat(c)
    return X[keep], x2d[:, keep], None if conf is None else conf[:, keep]


def pose_distance(R, t, R_true, t_true):
    """||R - R*||_F + ||t - t*||, per problem"""
    return np.sqrt(((R - R_true) ** 2).sum(axis=(-2, -1))) + np.sqrt(((t - t_true) ** 2).sum(axis=-1))
