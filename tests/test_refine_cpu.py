"""CPU: the float64 restatement of the camera-and-points refinement (tests/refine_restated.py; rules: DESIGN §2 "Camera +
points refinement") on the inputs of tests/refine_cases.py: the Schur step against a dense solve, the analytic Jacobians
against central differences, the whole solver against scipy's least_squares from the same start, the stability of the
stopping point under a change of the last bits of the start (rule 9's protocol), noise-free keypoints, the limit of a
stiff prior (the resection's cameras), soft_l1 against linear under gross outliers, and the masking rule.  The kernel is
held to this restatement by tests/test_refine_gpu.py."""
import numpy as np
import pytest

import refine_cases as fc
import refine_restated as fr
import resect_restated as rr

SMALL = [x for x in fc.cases() if not x[0].startswith("n1100")]        # scipy differentiates densely: 12 + 3 n columns
# (c): the worst differences measured over SMALL (printed by the test), and the bounds at ten times those
SCIPY_BOUNDS = dict(params=10 * 1.48e-7, cost=10 * 2.03e-11, err=10 * 1.77e-5)
# (f): lambda_x = 1e12 against the resection from the same start, worst |dR|, |dt| measured 4.33e-6 (step_V4_lx100_soft)
STIFF_PRIOR_BOUND = 10 * 4.33e-6


def run(c, kw, **over):
    X, x2d, conf = fc.flat(c)
    return fr.refine_cameras_points(X, x2d, conf=conf, **dict(kw, **over))


@pytest.mark.parametrize("lambda_x,loss", [(0.0, "linear"), (1.0, "linear"), (100.0, "soft_l1")])
def test_schur_step_equals_the_dense_solve(lambda_x, loss):
    """(a) n = 8, V = 2: (H + lam I) delta = -g solved through the Schur complement on the points against numpy's dense
    solve of the 36 x 36 system, within 1e-10 (1 + |x|) (measured: 1e-12), at lam0 = 1e-3 max diag H and, with a prior, at
    rule 9's floor 1e-9 max diag H.  Without a prior H is singular along the seven gauge directions, so at the floor the
    system's condition number is 1e9 and neither solve is good to 1e-10 (they differ by 1.4e-9 on a step 0.1 long): that
    lam is compared where the prior bounds the condition."""
    c = fc.rig(T=1, V=2, seed=81, joints=8)
    R0, t0 = fc.start(c, False)
    X, x2d, _ = fc.flat(c)
    Xs = X + 0.01 * np.random.default_rng(1).normal(0, 1, X.shape)      # off the prior's centre: its gradient is not zero
    lin = fr.linearise(c["K"], R0[0], t0[0], Xs, X, x2d, np.ones(x2d.shape[:2]), lambda_x, loss, fc.F_SCALE)
    H, g = fr.dense_system(lin)
    assert H.shape == (36, 36) and np.abs(H - H.T).max() <= 1e-13 * np.abs(H).max()
    for lam in (1e-3 * fr.max_diag(lin),) + ((1e-9 * fr.max_diag(lin),) if lambda_x > 0 else ()):
        dc, dX = fr.schur_step(lin, lam)
        want = np.linalg.solve(H + lam * np.eye(36), -g)
        got = np.concatenate([dc.ravel(), dX.ravel()])
        print(lambda_x, loss, lam, np.abs(got - want).max())
        assert (np.abs(got - want) <= 1e-10 * (1 + np.abs(want))).all()


@pytest.mark.parametrize("lambda_x,loss", [(0.0, "linear"), (4.0, "linear"), (4.0, "soft_l1")])
def test_analytic_jacobians_against_central_differences(lambda_x, loss):
    """(b) H = J^T rho' J and g = J^T rho' r of rule 6 against the Jacobian of the residual vector by central differences
    in (omega_v, dt_v, dX_i) with R = Exp(omega) R0 (h = 1e-6: truncation 1e-12 relative, rounding 1e-9): relative 1e-6"""
    c = fc.rig(T=1, V=2, seed=82, joints=7, with_conf=True)
    R0, t0 = fc.start(c, False)
    X, x2d, conf = fc.flat(c)
    K, R, t, w = c["K"], R0[0], t0[0], conf
    Xs = X + 0.01 * np.random.default_rng(2).normal(0, 1, X.shape)
    n, V = X.shape[0], 2
    sl = np.sqrt(lambda_x)

    def res(p):
        Xp = Xs + p[6 * V:].reshape(n, 3)
        out = []
        if lambda_x > 0:
            out.append((sl * (Xp - X)).ravel())
        for v in range(V):
            r = rr.residuals(K[v], rr.exp_so3(p[6 * v:6 * v + 3]) @ R[v], t[v] + p[6 * v + 3:6 * v + 6], Xp, x2d[v], w[v])[4]
            out.append(r.ravel())
        return np.concatenate(out)

    m = 6 * V + 3 * n
    h = 1e-6
    Jn = np.stack([(res(h * e) - res(-h * e)) / (2 * h) for e in np.eye(m)], axis=1)
    r0 = res(np.zeros(m))
    rho1 = fr.rho(r0, loss, fc.F_SCALE)[0]
    lin = fr.linearise(K, R, t, Xs, X, x2d, w, lambda_x, loss, fc.F_SCALE)
    H, g = fr.dense_system(lin)
    Hn, gn = Jn.T @ (rho1[:, None] * Jn), Jn.T @ (rho1 * r0)
    print(np.abs(H - Hn).max() / np.abs(H).max(), np.abs(g - gn).max() / np.abs(g).max())
    assert np.abs(H - Hn).max() <= 1e-6 * np.abs(H).max() and np.abs(g - gn).max() <= 1e-6 * np.abs(g).max()
    half = 0.5 * fc.F_SCALE ** 2 if loss == "soft_l1" else 0.5
    assert abs(lin["cost"] - half * fr.rho(r0, loss, fc.F_SCALE)[1].sum()) <= 1e-12 * lin["cost"]


def scipy_solve(K, R0, t0, X0, x, w, lambda_x, loss, f_scale):
    """the reference's call (slove_rt_from_3d.py:236-244) on its stacked residuals [w_v (proj_v - x_v), sqrt(lambda_x)
    (X - X0)] (:140-168) over x0 = pack(init, X), with the tolerances at 1e-15; cv2.Rodrigues / projectPoints are scipy's
    Rotation.from_rotvec and K (R X + t) divided by its third component, written out here: nothing of the restatement.
    jac="3-point": with the default forward differences scipy stops 3.5e-11 short in cost (step_V3_lx1), which under a
    prior of lambda_x = 1 leaves its parameters 8.7e-5 from the minimum; with central differences they agree to 1e-7"""
    from scipy.optimize import least_squares
    from scipy.spatial.transform import Rotation

    V, n = x.shape[:2]

    def fun(p):
        X = p[6 * V:].reshape(n, 3)
        out = []
        for v in range(V):
            Xc = X @ Rotation.from_rotvec(p[6 * v:6 * v + 3]).as_matrix().T + p[6 * v + 3:6 * v + 6]
            xh = Xc @ K[v].T
            out.append(np.repeat(w[v], 2) * (xh[:, :2] / xh[:, 2:3] - x[v]).reshape(-1))
        if lambda_x > 0:
            out.append(np.sqrt(lambda_x) * (X - X0).reshape(-1))
        return np.concatenate(out)

    x0 = np.concatenate([np.concatenate([Rotation.from_matrix(R0[v]).as_rotvec(), t0[v]]) for v in range(V)] + [X0.reshape(-1)])
    r = least_squares(fun, x0, method="trf", jac="3-point", loss=loss, f_scale=f_scale, max_nfev=200, xtol=1e-15, ftol=1e-15,
                      gtol=1e-15)
    return (np.stack([Rotation.from_rotvec(r.x[6 * v:6 * v + 3]).as_matrix() for v in range(V)]),
            np.stack([r.x[6 * v + 3:6 * v + 6] for v in range(V)]), r.x[6 * V:].reshape(n, 3), r.cost)


def test_restatement_against_scipy_least_squares():
    """(c) From the same start, every group of every case up to 65 points: with lambda_x > 0 R, t and X_opt of the
    restatement's Levenberg-Marquardt and of scipy's trf on the reference's residual function, same loss and f_scale;
    with lambda_x = 0, where the two end at different points of the gauge orbit (0.31 apart, step_V3_lx0_conf), the
    cost (relative) and the errors; cost and err are compared on the lambda_x > 0 cases too.  Measured worst: parameters
    1.48e-7 (n6_V2_lx1), cost 2.03e-11 relative to max(cost, 1) and err 1.77e-5 px (both step_V2_lx0_soft); the bounds are
    ten times those.  Cost and err are what rule 8's tau = 3e-8 leaves: the restatement stops on a step of 1e-6, scipy
    goes on (at tau = 1e-12 the three figures were 1.31e-7, 6.8e-14 and 2.48e-7 px, but then whether a lambda_x = 0 case
    stops at all depends on the last bits of its start: see DESIGN)."""
    worst = dict(params=0.0, cost=0.0, err=0.0)
    for name, c, kw in SMALL:
        X, x2d, conf = fc.flat(c)
        got = run(c, kw)
        w_all, _ = rr.weights_and_mask(X, x2d, conf, 0.0)
        gs = kw["group_size"] or X.shape[0]
        wn = dict(params=0.0, cost=0.0, err=0.0)
        for g in range(X.shape[0] // gs):
            sl = slice(g * gs, (g + 1) * gs)
            Rs, ts, Xs, cs = scipy_solve(got["K"][g], kw["R0"][g], kw["t0"][g], X[sl], x2d[:, sl], w_all[:, sl], kw["lambda_x"],
                                         kw["loss"], kw["f_scale"])
            if kw["lambda_x"] > 0:
                wn["params"] = max(wn["params"], np.abs(Rs - got["R"][g]).max(), np.abs(ts - got["t"][g]).max(),
                                   np.abs(Xs - got["X_opt"][sl]).max())
            wn["cost"] = max(wn["cost"], abs(cs - got["cost"][g]) / max(got["cost"][g], 1.0))
            for v in range(c["V"]):
                d = rr.project(got["K"][g, v], Rs[v], ts[v], Xs) - x2d[v, sl]
                wn["err"] = max(wn["err"], np.abs(np.sqrt((d * d).sum(axis=1)) - got["err"][v, sl]).max())
        print(f"{name}: " + ", ".join(f"{k} {v:.2e}" for k, v in wn.items()))
        worst = {k: max(worst[k], wn[k]) for k in worst}
    print("worst:", worst)
    for k in worst:
        assert worst[k] <= SCIPY_BOUNDS[k], worst


@pytest.mark.parametrize("case", fc.prior_cases(), ids=lambda c: c[0])
def test_rule_9_stopping_point_does_not_depend_on_the_last_bits_of_the_start(case):
    """(d) Every case with lambda_x > 0 stops on the step criterion before max_evals (rule 9 (a)), and the start moved by
    1e-13 relative moves the final R, t, X_opt by less than 1e-10 (rule 9 (b); measured: 4.9e-12 at tau = 3e-8,
    lambda_min = 1e-9).  The protocol is that of tests/test_resect_cpu.py.  The points are part of the start as well: begun
    1e-13 relative off X, with X still the prior's centre, they end within 1e-10 too (measured: 2.1e-13, step_V3_lx1)."""
    name, c, kw = case
    rng = np.random.default_rng(0)
    a = run(c, kw)
    b = run(c, kw, R0=kw["R0"] * (1 + 1e-13 * rng.uniform(-1, 1, kw["R0"].shape)),
            t0=kw["t0"] * (1 + 1e-13 * rng.uniform(-1, 1, kw["t0"].shape)))
    assert a["success"].all() and b["success"].all() and (a["n_evals"] < 200).all()
    move = max(np.abs(a[k] - b[k]).max() for k in ("R", "t", "X_opt"))
    print(name, move, "evaluation counts equal:", np.array_equal(a["n_evals"], b["n_evals"]))
    assert move < 1e-10
    # the points are part of the start too: they begin 1e-13 relative off X, which stays the prior's centre
    X = fc.flat(c)[0]
    p = run(c, kw, Xs=X * (1 + 1e-13 * rng.uniform(-1, 1, X.shape)))
    move_x = max(np.abs(a[k] - p[k]).max() for k in ("R", "t", "X_opt"))
    print(name, "points moved:", move_x)
    assert p["success"].all() and move_x < 1e-10


@pytest.mark.parametrize("case", [x for x in fc.cases() if x[2]["lambda_x"] == 0 and x[2]["K"] is not None], ids=lambda c: c[0])
def test_gauge_invariant_outputs_are_stable_without_a_prior(case):
    """rule 9 at lambda_x = 0: under the same change of the start every group still stops on the step criterion (the
    accepted steps that rounding in g keeps alive along the gauge are at most 1.4e-9 (1 + ||(t, X)||) at lambda_min = 1e-9,
    a 22nd of tau), the cost moves by less than 1e-10 relative and err by less than 1e-9 px (measured: 8.9e-12 and
    2.6e-12)"""
    name, c, kw = case
    rng = np.random.default_rng(0)
    a = run(c, kw)
    b = run(c, kw, R0=kw["R0"] * (1 + 1e-13 * rng.uniform(-1, 1, kw["R0"].shape)),
            t0=kw["t0"] * (1 + 1e-13 * rng.uniform(-1, 1, kw["t0"].shape)))
    print(name, np.abs(a["cost"] - b["cost"]).max(), np.nanmax(np.abs(a["err"] - b["err"])))
    assert a["success"].all() and b["success"].all()
    assert (np.abs(a["cost"] - b["cost"]) <= 1e-10 * np.maximum(a["cost"], 1.0)).all()
    assert np.nanmax(np.abs(a["err"] - b["err"])) < 1e-9


@pytest.mark.parametrize("case", [x for x in fc.cases() if x[2]["lambda_x"] == 0 and x[2]["K"] is not None], ids=lambda c: c[0])
def test_noise_free_keypoints_are_met_from_a_perturbed_start(case):
    """(e) lambda_x = 0, noise-free keypoints, cameras started ~0.01 rad / 3 cm off and points 5 cm off: max_err < 1e-8 px
    (measured: 2.6e-10, step_V2_lx0)"""
    name, c, kw = case
    X, x2d, conf = fc.flat(c)
    got = fr.refine_cameras_points(X, c["clean"].reshape(c["V"], -1, 2), conf=conf, **kw)
    print(name, got["max_err"].max(), got["n_evals"])
    assert got["success"].all() and got["max_err"].max() < 1e-8


@pytest.mark.parametrize("case", fc.prior_cases(), ids=lambda c: c[0])
def test_a_stiff_prior_returns_the_resections_cameras(case):
    """(f) lambda_x = 1e12 holds the points (they move by under 1.1e-8) and the cameras are those of the resection
    restatement from the same start: measured worst 4.33e-6 (step_V4_lx100_soft), bound ten times that.  The prior's 1e12
    is then the largest diagonal entry of H, so rule 9's floor holds lambda at 1e3, against camera blocks of 1e5 to 1e7,
    and the last steps shrink slowly: rule 8 stops them 4e-6 short (1.64e-8 at tau = 1e-12)"""
    name, c, kw = case
    X, x2d, conf = fc.flat(c)
    got = run(c, kw, lambda_x=1e12)
    ref = rr.resect_cameras(X, x2d, conf=conf, K=kw["K"], group_size=kw["group_size"], R0=kw["R0"], t0=kw["t0"], loss=kw["loss"],
                            f_scale=kw["f_scale"])
    d = max(np.abs(got["R"] - ref["R"]).max(), np.abs(got["t"] - ref["t"]).max())
    print(name, d, got["moved"].max())
    assert d <= STIFF_PRIOR_BOUND and got["moved"].max() < 1e-6


@pytest.mark.parametrize("seed", [71, 72])
def test_soft_l1_ends_nearer_the_true_relative_pose_than_linear(seed):
    """(g) The whole-clip case (T = 243, J = 17, one group) with 10 % keypoints moved by sigma = 80 px, lambda_x = 100:
    ||R_rel - R*||_F + ||t_rel - t*|| of soft_l1 (f_scale 2) is under that of linear.  Measured with this restatement on
    seeds 71, 72, 73: 0.37 / 0.33 / 0.41 against 1.17 / 0.74 / 1.82 (at lambda_x = 1: 0.73 / 0.76 / 0.62 against
    1.19 / 0.77 / 1.77).  With the points free an outlier in one of two views is absorbed by its point up to the
    epipolar constraint, so the gap is smaller than the resection's; the prior is what restores it."""
    c, kw = fc.clip_outlier_case(seed)
    X, x2d, _ = fc.flat(c)
    Rt, tt = fc.true_relative(c)
    d = []
    for loss in ("linear", "soft_l1"):
        r = fr.refine_cameras_points(X, x2d, lambda_x=100.0, loss=loss, f_scale=fc.F_SCALE, **kw)
        d.append(float(fc.pose_distance(r["R_rel"][0, 1], r["t_rel"][0, 1], Rt, tt)))
    print(seed, d)
    assert d[1] < d[0]


def test_masked_points_keep_X_and_a_group_with_five_points_fails():
    """rule 1 and rule 10: a masked point of each kind keeps its X bit for bit, a group with 5 usable points fails with
    X_opt = X, and a masked point equals its removal"""
    name, c, kw, n_points, masked = fc.masked_case()
    X, x2d, conf = fc.flat(c)
    got = run(c, kw)
    assert np.array_equal(got["n_points"], n_points)
    bad = n_points < rr.MIN_POINTS
    assert np.array_equal(got["success"] == 0, bad)
    for key in ("R", "t", "cost0", "cost", "mean_err", "rms_err", "max_err", "moved", "R_rel", "t_rel"):
        assert np.isnan(got[key][bad]).all() and np.isfinite(got[key][~bad]).all(), key
    _, used = rr.weights_and_mask(X, x2d, conf, fc.MIN_CONF)
    used = used & np.repeat(~bad, fc.J)
    assert np.array_equal(got["X_opt"].view(np.uint64)[~used], X.view(np.uint64)[~used])
    assert np.array_equal(~np.isnan(got["err"]), np.stack([used, used]))
    g0 = 0
    keep = np.zeros(X.shape[0], bool)
    keep[g0 * fc.J:(g0 + 1) * fc.J] = used[g0 * fc.J:(g0 + 1) * fc.J]
    alone = fr.refine_cameras_points(X[keep], x2d[:, keep], conf=conf[:, keep], **dict(kw, group_size=None, R0=kw["R0"][:1], t0=kw["t0"][:1]))
    for key in ("R", "t", "cost"):
        assert np.allclose(alone[key][0], got[key][g0], rtol=0, atol=1e-12), key
    assert np.allclose(alone["X_opt"], got["X_opt"][keep], rtol=0, atol=1e-12)
