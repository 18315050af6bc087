"""CPU: the float64 restatement of the camera resection (tests/resect_restated.py; rules: DESIGN §2 "Resection") on the
inputs of tests/resect_cases.py: against scipy's least_squares from the same start, against the truth on noise-free data,
soft_l1 against linear under gross outliers, the stability of the stopping point under a change of the last bits of the
start, and the masking rule.  The kernel is held to this restatement by tests/test_resect_gpu.py."""
import numpy as np
import pytest

import resect_cases as rc
import resect_restated as rr

ALL = rc.cases() + [rc.given_start_case()[:4], rc.masked_case()[:4]]

# (a): worst |R - R_scipy|, |t - t_scipy| measured over ALL (printed by the test), and the bound at ten times that: scipy
# stops by its own criteria and differentiates numerically
SCIPY_WORST_MEASURED = 3.83e-8
SCIPY_BOUND = 10 * SCIPY_WORST_MEASURED


def run(c, kw, groups, **over):
    X, x2d, conf = rc.flat(c)
    return rr.resect_cameras(X, x2d, conf=conf, groups=groups, **dict(kw, **over))


def scipy_solve(K, R0, t0, X, x, w, loss, f_scale):
    """the reference's call (slove_rt_from_3d.py:239-244) on its stacked residuals [w_v (proj_v - x_v)] over the views, with
    the tolerances at 1e-15; cv2.Rodrigues / projectPoints are scipy's Rotation.from_rotvec and K (R X + t) divided by its
    third component, written out here"""
    from scipy.optimize import least_squares
    from scipy.spatial.transform import Rotation

    V = len(K)

    def project_points(rvec, tvec, Kv):      # cv2.projectPoints without distortion, written out: nothing of the restatement
        Xc = X @ Rotation.from_rotvec(rvec).as_matrix().T + tvec
        xh = Xc @ Kv.T                       # the whole 3 x 3 K
        return xh[:, :2] / xh[:, 2:3]

    def fun(p):
        return np.concatenate([(np.repeat(w[v], 2) * (project_points(p[6 * v:6 * v + 3], p[6 * v + 3:6 * v + 6], K[v]) - x[v]).reshape(-1))
                               for v in range(V)])

    x0 = np.concatenate([np.concatenate([Rotation.from_matrix(R0[v]).as_rotvec(), t0[v]]) for v in range(V)])
    r = least_squares(fun, x0, method="trf", loss=loss, f_scale=f_scale, max_nfev=200, xtol=1e-15, ftol=1e-15, gtol=1e-15)
    return (np.stack([Rotation.from_rotvec(r.x[6 * v:6 * v + 3]).as_matrix() for v in range(V)]),
            np.stack([r.x[6 * v + 3:6 * v + 6] for v in range(V)]))


def test_restatement_against_scipy_least_squares():
    """(a) From the same start (the restatement's own: the DLT resection or the given R0, t0), on every case and every
    compared group: R and t of the restatement's Levenberg-Marquardt and of scipy's trf on the reference's residual
    function, same loss and f_scale.  Measured worst difference 3.83e-8 (out10_T64_V2_step_linear: 17 points with gross
    outliers under the linear loss, the flattest minima of the set; the noise-free cases agree to 6e-15, the whole-clip
    cases to 2.5e-9, the other per-step cases to 3.7e-8); bound 3.83e-7 = 10 x that."""
    worst = {}
    for name, c, kw, groups in ALL:
        X, x2d, conf = rc.flat(c)
        got = run(c, kw, groups)
        start = run(c, kw, groups, max_evals=1)
        w_all, used_all = rr.weights_and_mask(X, x2d, conf, kw.get("min_conf", 0.0))
        gs = kw["group_size"] or X.shape[0]
        worst[name] = 0.0
        for g in groups:
            if got["n_points"][g, 0] < rr.MIN_POINTS:
                continue
            sl = slice(g * gs, (g + 1) * gs)
            u = used_all[sl]
            Rs, ts = scipy_solve(got["K"][g], start["R"][g], start["t"][g], X[sl][u], x2d[:, sl][:, u], w_all[:, sl][:, u],
                                 kw["loss"], kw.get("f_scale", 1.0))
            worst[name] = max(worst[name], np.abs(Rs - got["R"][g]).max(), np.abs(ts - got["t"][g]).max())
        print(f"{name}: {worst[name]:.2e}")
    print("worst:", max(worst.values()))
    assert max(worst.values()) <= SCIPY_BOUND, worst


@pytest.mark.parametrize("case", rc.clean_cases(), ids=lambda c: c[0])
def test_noise_free_cases_recover_the_truth(case):
    """(b) R, t of the truth within 1e-9 (1 + |x|) (measured: 6e-15)"""
    name, c, kw, groups = case
    got = run(c, kw, groups)
    g = np.array(groups)
    assert got["success"][g].all() and (got["n_points"][g] == (kw["group_size"] or c["T"] * rc.J)).all()
    for key in ("R", "t"):
        d = np.abs(got[key][g] - c[key])
        print(name, key, d.max())
        assert (d <= 1e-9 * (1 + np.abs(c[key]))).all()
    assert np.nanmax(got["max_err"][g]) <= 1e-9


@pytest.mark.parametrize("case", rc.outlier_pairs(), ids=lambda c: c[0])
def test_soft_l1_ends_closer_to_the_truth_than_linear(case):
    """(c) Under 5 and 10 % keypoints moved by sigma = 80 px, per problem, no exception allowed: the distance
    ||R - R*||_F + ||t - t*|| of soft_l1 is strictly under that of linear (whole clips, from the DLT start: 2.7e-4 .. 1.8e-2
    against 7.6e-3 .. 1.4e-1).

    The per-step case (17 points a problem, one to four of them moved) is held to the same claim, on all 64 steps and
    every problem with a moved keypoint (109 of 128; a problem without one is not an outlier case: there either loss may
    end nearer), from the given start R0, t0 near the pose (rc.start_near_truth).  From the DLT start the claim does NOT
    hold there, and the test says so by asserting what happens instead: the unweighted DLT of 17 points is carried off by
    a single keypoint moved by 80 px, 19 of the 109 problems then start beyond the reach of either loss and both end at
    the same far local minimum (distance > 10 for both), where which is nearer means nothing.  Wherever linear ends
    within 1 of the pose, soft_l1 is strictly nearer from the DLT start too.  DESIGN §2 "Resection" states this limit."""
    name, c, kw_lin, kw_soft, groups = case
    if kw_lin["group_size"] is None:
        g = np.array(groups)
        d = [rc.pose_distance(r["R"][g], r["t"][g], c["R"], c["t"]) for r in (run(c, kw_lin, groups), run(c, kw_soft, groups))]
        print(name, "linear", d[0].min(), d[0].max(), "soft_l1", d[1].min(), d[1].max())
        assert (d[1] < d[0]).all()
        return
    G = c["T"]
    every = list(range(G))
    hit = c["moved"].sum(axis=2).T > 0                      # [T, V]: the problem has a moved keypoint
    R0, t0 = rc.start_near_truth(c, G, 77)
    d = [rc.pose_distance(r["R"], r["t"], c["R"], c["t"]) for r in (run(c, kw_lin, every, R0=R0, t0=t0), run(c, kw_soft, every, R0=R0, t0=t0))]
    exceptions = int((d[1] >= d[0])[hit].sum())
    print(name, "given start: problems", int(hit.sum()), "exceptions", exceptions, "medians", np.median(d[0][hit]), np.median(d[1][hit]))
    assert hit.sum() >= 100 and exceptions == 0
    d = [rc.pose_distance(r["R"], r["t"], c["R"], c["t"]) for r in (run(c, kw_lin, every), run(c, kw_soft, every))]
    lost = hit & (d[1] >= d[0])
    print(name, "DLT start: exceptions", int(lost.sum()), "their distances", d[0][lost].min(initial=np.inf), d[1][lost].min(initial=np.inf))
    assert (d[0][lost] > 10).all() and (d[1][lost] > 10).all()
    near = hit & (d[0] < 1)
    assert near.sum() >= 60 and (d[1][near] < d[0][near]).all()


@pytest.mark.parametrize("case", ALL, ids=lambda c: c[0])
def test_rule_5_stopping_point_does_not_depend_on_the_last_bits_of_the_start(case):
    """(d) The start moved by 1e-13 relative moves the final R, t by at most 1e-11 (measured: 4.3e-13, the noise-free cases
    included).  What makes it so is that the cost change of a trial is formed from the step (rr.cost_change): taken as
    the difference of two rounded costs, whose own rounding at 17 points, K ~ 1100 px and 1 px residuals is 3e-14
    relative, above the 1e-14 slack of the acceptance test, the same perturbation moved t by 1.2e-9
    (noise1_T64_V2_step_conf) and changed the evaluation counts."""
    name, c, kw, groups = case
    start = run(c, kw, groups, max_evals=1)
    rng = np.random.default_rng(0)
    kw = {k: v for k, v in kw.items() if k not in ("R0", "t0")}
    R0, t0 = np.nan_to_num(start["R"]), np.nan_to_num(start["t"])
    a = run(c, kw, groups, R0=R0, t0=t0)
    b = run(c, kw, groups, R0=R0 * (1 + 1e-13 * rng.uniform(-1, 1, R0.shape)), t0=t0 * (1 + 1e-13 * rng.uniform(-1, 1, t0.shape)))
    g = np.array(groups)
    assert np.array_equal(a["success"][g], b["success"][g])
    ok = a["success"][g].astype(bool)
    move = max(np.abs(a["R"][g][ok] - b["R"][g][ok]).max(), np.abs(a["t"][g][ok] - b["t"][g][ok]).max())
    print(name, move, "evaluation counts equal:", np.array_equal(a["n_evals"][g], b["n_evals"][g]))
    assert move <= 1e-11


def test_group_with_five_points_fails_and_its_neighbours_do_not():
    """(e) and rule 1: X non-finite, a keypoint non-finite in ONE view, a weight under min_conf in ONE view each mask the
    point in EVERY view; scores are clipped to [0, 1] with non-finite -> 0"""
    name, c, kw, groups, n_points = rc.masked_case()
    got = run(c, kw, groups)
    assert np.array_equal(got["n_points"], np.stack([n_points, n_points], axis=1))
    bad = n_points < rr.MIN_POINTS
    assert bad.sum() == 1 and np.array_equal(got["success"][:, 0] == 0, bad)
    for key in ("R", "t", "cost0", "cost", "mean_err", "rms_err", "max_err", "R_rel", "t_rel"):
        assert np.isnan(got[key][bad]).all() and np.isfinite(got[key][~bad]).all(), key
    assert np.isfinite(got["K"]).all() and (got["n_evals"][bad] == 0).all()
    X, x2d, conf = rc.flat(c)
    _, used = rr.weights_and_mask(X, x2d, conf, rc.MIN_CONF)
    used = used & np.repeat(~bad, rc.J)
    assert np.array_equal(~np.isnan(got["err"]), np.stack([used, used]))
    # a masked point equals its removal
    g0 = 0
    sl = slice(g0 * rc.J, (g0 + 1) * rc.J)
    keep = np.zeros(X.shape[0], bool)
    keep[sl] = used[sl]
    Xr, xr, cr = rc.removed(c, keep)
    alone = rr.resect_cameras(Xr, xr, conf=cr, K=c["K"], loss="linear", min_conf=rc.MIN_CONF)
    for key in ("R", "t", "cost"):
        assert np.allclose(alone[key][0], got[key][g0], rtol=0, atol=1e-12), key


def test_inferred_K_is_the_references_formula():
    """rule 2 against infer_K_from_2d (slove_rt_from_3d.py:65-73) written out with NumPy's mean and std"""
    x = rc.rig(T=4, V=2, seed=3, noise=1.0)["x2d"][0].reshape(-1, 2)
    K = rr.infer_K(x)
    f = max(x[:, 0].std() + 1e-6, x[:, 1].std() + 1e-6) * 2.0
    assert np.allclose(K, [[f, 0, x[:, 0].mean()], [0, f, x[:, 1].mean()], [0, 0, 1]], rtol=1e-14, atol=0)


def test_dlt_start_is_a_rotation_near_the_pose():
    c = rc.rig(T=4, V=2, seed=5, noise=1.0)
    X, x2d, _ = rc.flat(c)
    R, t = rr.dlt_init(c["K"][0], X, x2d[0])
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-12 and np.linalg.det(R) > 0
    assert rc.pose_distance(R, t, c["R"][0], c["t"][0]) < 0.2
