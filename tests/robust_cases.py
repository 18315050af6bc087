"""The inputs of the robust-triangulation tests, NumPy only, so that tests/test_robust_cpu.py (which checks the margins on
the restatement) and tests/test_robust_gpu.py (which runs the kernel) see the same arrays.  Every array is rounded to
float32 before anyone uses it: that is what the kernel reads.

The rig is the camera arc, the intrinsics and the joint cloud of tests/test_person_gpu.py::_rig restated (that function
uploads to the device, so it cannot be imported here), with plain 0.5 px Gaussian keypoint noise."""
import numpy as np


def _f32(a):
    return np.asarray(a, np.float64).astype(np.float32)


def rotvec_matrix(r):
    """Rodrigues: rotation vector -> matrix"""
    r = np.asarray(r, np.float64)
    th = np.linalg.norm(r)
    if th < 1e-12:
        return np.eye(3)
    k = r / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)


def rig(V, J, T, rng, noise=0.5):
    """T steps of V cameras on an arc looking at J points near the origin -> float64 K, R [T, V, 3, 3], t [T, V, 3],
    keypoints [T, V, J, 2] = projections + noise, the true points X [T, J, 3]"""
    K, R, t = np.empty((T, V, 3, 3)), np.empty((T, V, 3, 3)), np.empty((T, V, 3))
    for i in range(T):
        for v in range(V):
            ang = (v - (V - 1) / 2) * 0.25 + rng.normal(scale=0.02)
            R[i, v] = rotvec_matrix([rng.normal(scale=0.02), ang, rng.normal(scale=0.02)])
            t[i, v] = [rng.normal(scale=0.1), rng.normal(scale=0.1), 6.0 + rng.normal(scale=0.2)]
            K[i, v] = [[600 + 10 * v, 0, 320], [0, 605 + 5 * v, 240], [0, 0, 1]]
    X = rng.normal(size=(T, J, 3)) * [0.5, 0.8, 0.4]
    kp = np.empty((T, V, J, 2))
    for i in range(T):
        for v in range(V):
            p = (X[i] @ R[i, v].T + t[i, v]) @ K[i, v].T
            kp[i, v] = p[:, :2] / p[:, 2:3]
    kp += rng.normal(scale=noise, size=kp.shape)
    return K, R, t, kp, X


def move_views(kp, rng, n_max, lo, hi):
    """per (step, joint): 0 .. n_max views, drawn without replacement, moved by lo .. hi px in a random direction ->
    (moved keypoints, bool [T, V, J] which were moved)"""
    T, V, J = kp.shape[:3]
    kp = kp.copy()
    moved = np.zeros((T, V, J), bool)
    for i in range(T):
        for j in range(J):
            n = rng.integers(0, n_max + 1)
            for v in rng.choice(V, n, replace=False):
                a, m = rng.uniform(0, 2 * np.pi), rng.uniform(lo, hi)
                kp[i, v, j] += [m * np.cos(a), m * np.sin(a)]
                moved[i, v, j] = True
    return kp, moved


def outlier_rig(V, J, seed, T=6, n_max=None, lo=25.0, hi=60.0):
    """The rig with outliers -> dict(K, R, t, kp, clean (the keypoints before anything was moved), conf: float32 arrays;
    moved: bool [T, V, J]; X_true).  Default: the gross-outlier rig, 0 .. min(2, V - 3) views per joint moved by
    25 .. 60 px.  conf: uniform scores in [0.2, 1] (some under the default threshold 0.3), drawn last."""
    rng = np.random.default_rng(seed)
    K, R, t, kp, X = rig(V, J, T, rng)
    n_max = max(0, min(2, V - 3)) if n_max is None else n_max
    moved_kp, moved = move_views(kp, rng, n_max, lo, hi)
    conf = rng.uniform(0.2, 1.0, (T, V, J))
    return dict(K=_f32(K), R=_f32(R), t=_f32(t), kp=_f32(moved_kp), clean=_f32(kp), conf=_f32(conf), moved=moved, X_true=X)


# Seeds.  Each was searched on the restatement alone, over seeds 100 V + J (+ 1000, 2000, ...), for what
# tests/test_robust_cpu.py then asserts of it: the gross rigs recover exactly the unmoved views; the moderate (8, 17) rig
# holds refits that change the inlier set, once and twice; the moderate (3, 12) rig with weighted refits holds refits that
# would leave fewer than two inliers; the V = 3 rig with one moved view holds winners picked by cost among equal counts.
SHAPES = [(2, 17), (3, 12), (4, 12), (8, 17)]
GROSS_SEEDS = {(2, 17): 217, (3, 12): 312, (4, 12): 412, (8, 17): 817}
MODERATE_SEEDS = {(3, 12): 312, (4, 12): 412, (8, 17): 817}
ONE_OF_THREE_SEED = 317
INLIER_PX = 3.0


def gross(V, J):
    return outlier_rig(V, J, GROSS_SEEDS[(V, J)])


def moderate(V, J):
    """0 .. min(3, V - 2) views per joint moved by 2 .. 7 px: around the 3 px threshold, so that refits change the set"""
    return outlier_rig(V, J, MODERATE_SEEDS[(V, J)], n_max=min(3, V - 2), lo=2.0, hi=7.0)


def one_of_three():
    """V = 3, 0 .. 1 views per joint moved by 25 .. 60 px: a pair that holds the moved view still has its own two views
    as inliers, so hypotheses of different sets share the winner's count and the cost decides"""
    return outlier_rig(3, 17, ONE_OF_THREE_SEED, n_max=1)


def hand_built():
    """name -> (case, use_conf, kwargs): the rules one by one on a small rig (V = 4, J = 8, T = 2; scores 0.9 unless said)"""
    def base(V=4, J=8, T=2, seed=44):
        c = outlier_rig(V, J, seed, T=T, n_max=0)
        c["conf"] = np.full(c["conf"].shape, 0.9, np.float32)
        return c

    out = {}
    c = base()
    c["kp"][0, 1, 2, 0] = np.nan                       # view 1 of joint 2: not eligible, its error NaN
    c["kp"][1, :, 5, 1] = np.nan                       # joint 5 of step 1: no eligible view at all
    c["kp"][1, 1:, 6, 0] = np.inf                      # joint 6 of step 1: one eligible view
    out["nan keypoint"] = (c, False, {})
    c = base()
    c["conf"][0, 2, 3] = 0.1                           # view 2 of joint 3 under the threshold: not eligible, error reported
    c["conf"][0, 1:, 4] = 0.1                          # joint 4: one eligible view -> fails
    c["conf"][1, 0, 0] = np.nan                        # a NaN score compares false
    out["low score"] = (c, True, {})
    c = base()
    flip = np.array([-1.0, 1.0, -1.0], np.float32)     # step 1: view 3 looks the other way, every joint is behind it
    c["R"][1, 3] = np.diag(flip) @ c["R"][1, 3]
    c["t"][1, 3] = flip * c["t"][1, 3]
    out["view behind"] = (c, False, {})
    c = base(V=2, J=8)
    c["kp"][0, 1, 1] += np.float32([0.0, 40.0])        # across the epipolar line: the two views cannot agree
    c["kp"][1, 0, 2] += np.float32([0.0, -25.0])
    out["two views"] = (c, False, {})
    c = base()
    c["conf"][0, 1, 1] = -0.5                          # eligible at conf_thr = -1, clipped to weight 0
    c["conf"][0, 2, 2] = np.inf                        # eligible, non-finite -> weight 0
    c["conf"][0, 0, 3] = 7.0                           # clipped to 1
    c["conf"][1, :, 4] = 0.0                           # all weights 0 -> refitted and refined unweighted
    c["conf"][1, 1:, 5] = -0.25                        # one positive weight -> unweighted as well
    c["conf"][1] *= np.linspace(0.4, 1.0, 4, dtype=np.float32)[:, None]
    out["zero weights"] = (c, True, dict(conf_thr=-1.0, weighted=True))
    c = gross(8, 17)
    c["K"][1, 3, 1, 1] = np.nan                        # step 1: view 3's seven pairs are skipped, the joints recovered
    out["nan camera"] = (c, False, dict(inlier_px=INLIER_PX))
    out["refined to the end"] = (gross(4, 12), False, dict(inlier_px=INLIER_PX, refine_iters=32))
    return out


BIG_T, BIG_SEED, BIG_SAMPLE = 4096, 40968, 64


def big():
    """T = 4096 steps at V = 8, J = 17 (one workgroup per step: the grid sizing) with gross outliers -> (case, the 64
    steps that are compared with the restatement)"""
    c = outlier_rig(8, 17, BIG_SEED, T=BIG_T)
    steps = np.sort(np.random.default_rng(BIG_SEED).choice(BIG_T, BIG_SAMPLE, replace=False))
    steps[0], steps[-1] = 0, BIG_T - 1
    return c, steps


def take_steps(c, steps):
    return {k: (v[steps] if isinstance(v, np.ndarray) else v) for k, v in c.items()}


def gpu_cases():
    """[(name, case, use_conf, kwargs)]: every input the GPU file runs the kernel on, so that the CPU file can check its
    margins first"""
    out = []
    for V, J in SHAPES:
        c = gross(V, J)
        for use_conf in (False, True):
            for weighted in (False, True):
                for refine_iters in (0, 5):
                    for min_inliers in sorted({2, min(3, V)}):
                        kw = dict(inlier_px=INLIER_PX, weighted=weighted, refine_iters=refine_iters, min_inliers=min_inliers)
                        out.append((f"gross V={V} J={J} conf={int(use_conf)} w={int(weighted)} gn={refine_iters} min={min_inliers}",
                                    c, use_conf, kw))
    for V, J in MODERATE_SEEDS:
        c = moderate(V, J)
        out.append((f"moderate V={V} J={J}", c, False, dict(inlier_px=INLIER_PX)))
        out.append((f"moderate V={V} J={J} weighted", c, True, dict(inlier_px=INLIER_PX, weighted=True)))
    out.append(("one of three moved", one_of_three(), False, dict(inlier_px=INLIER_PX)))
    for name, (c, use_conf, kw) in hand_built().items():
        out.append((f"hand-built: {name}", c, use_conf, kw))
    return out
