"""CPU: the float64 restatement of the robust triangulation (tests/robust_restated.py) against independent statements
of its parts, its rules one by one on hand-built inputs, the recovery property it exists for, the margins of every
input the GPU file runs the kernel on (tests/robust_cases.py), the data-dependent branches each forced by an input and
asserted to have been taken, and the argument checks of the new entry points (no GPU: nothing is launched).

The tests of the restatement alone use nothing of the feature but these new files: they make the yardstick trustworthy
before a kernel is measured with it.  The argument checks need the feature itself."""
import ctypes

import numpy as np
import pytest
import torch

import robust_cases as rc
import robust_restated as rr
from skiing_analysis_pytorch_amd import _lib, geometry, infer

f64 = lambda a: np.asarray(a, np.float64)   # noqa: E731


def run(c, use_conf=False, **kw):
    return rr.triangulate_robust(f64(c["K"]), f64(c["R"]), f64(c["t"]), f64(c["kp"]), f64(c["conf"]) if use_conf else None, **kw)


def step_P(c, i):
    return rr.cameras(f64(c["K"][i]), f64(c["R"][i]), f64(c["t"][i]))


def close(a, b, tol=1e-9):
    a, b = f64(a), f64(b)
    return bool((np.abs(a - b) <= tol * (1 + np.abs(b))).all())


def svd_dlt(P, kp):
    """the system of vggt/triangulate.py:19-34 over all views, solved by an SVD of the unsquared A"""
    A = np.concatenate([np.stack([kp[v, 0] * P[v, 2] - P[v, 0], kp[v, 1] * P[v, 2] - P[v, 1]]) for v in range(len(P))])
    X = np.linalg.svd(A)[2][-1]
    return X[:3] / X[3]


# ---- the restatement against independent statements of its parts ------------------------------------------------------
@pytest.mark.parametrize("V,J", [(2, 17), (3, 12), (8, 17)])
def test_all_inliers_unrefined_is_the_svd_dlt_over_all_views(V, J):
    c = rc.outlier_rig(V, J, 5 * V + J, n_max=0)
    res = run(c, inlier_px=rc.INLIER_PX, refine_iters=0)
    assert (res["inlier_views"] == (1 << V) - 1).all() and res["ok"].all()
    for i in range(len(c["kp"])):
        P = step_P(c, i)
        for j in range(J):
            assert close(res["joints3d"][i, j], svd_dlt(P, f64(c["kp"][i, :, j]))), (i, j)


def test_refinement_is_the_least_squares_minimiser_and_has_converged_after_five_steps():
    from scipy.optimize import least_squares
    c = rc.gross(8, 17)
    r0 = run(c, inlier_px=rc.INLIER_PX, refine_iters=0)
    r5 = run(c, inlier_px=rc.INLIER_PX, refine_iters=5)
    r10 = run(c, inlier_px=rc.INLIER_PX, refine_iters=10)
    # five steps have converged: five more move X by rounding only.  Not bit for bit: the decrease test is formed from
    # the step (robust_restated.cost_change), so it goes on accepting steps of a few ulp, each of which does lower c as
    # evaluated at that X; the noise of a residual, 3e-14 px, over sqrt(lambda_min(H)) ~ 17 px per unit is 2e-15 a step
    print(f"refine_iters 5 against 10: {np.abs(r5['joints3d'] - r10['joints3d']).max():.2e}")
    assert close(r5["joints3d"], r10["joints3d"], 1e-12)
    assert np.array_equal(r5["inlier_views"], r0["inlier_views"])          # the set is not re-thresholded
    gap, w = 0.0, np.ones(8)
    for i in range(6):
        P = step_P(c, i)
        for j in range(17):
            kp, inl = f64(c["kp"][i, :, j]), r0["joints"][i][j]["inliers"]
            sol = least_squares(lambda X: rr.residuals(P, kp, w, inl, X), r0["joints3d"][i, j], method="trf", jac="3-point",
                                xtol=1e-15, ftol=1e-15, gtol=1e-15)     # central differences: forward ones stop 3e-9 short
            assert close(r5["joints3d"][i, j], sol.x), (i, j, np.abs(r5["joints3d"][i, j] - sol.x).max())
            gap = max(gap, float(np.linalg.norm(r5["joints3d"][i, j] - r0["joints3d"][i, j])))
    print(f"largest distance of the DLT refit from the reprojection minimiser: {gap * 1e3:.3f} mm")
    assert gap > 1e-4        # the refinement is not a no-op: the algebraic minimiser is tenths of a millimetre off


def test_weighted_refinement_minimises_the_weighted_residuals():
    from scipy.optimize import least_squares
    c = rc.moderate(4, 12)
    res = run(c, True, inlier_px=rc.INLIER_PX, weighted=True, refine_iters=8)
    n = 0
    for i in range(6):
        P = step_P(c, i)
        for j in range(12):
            r = res["joints"][i][j]
            if r["failed"]:
                continue
            w = rr.set_weights(rr.weights(f64(c["conf"][i, :, j]), True, 4), r["inliers"])
            kp = f64(c["kp"][i, :, j])
            sol = least_squares(lambda X: rr.residuals(P, kp, w, r["inliers"], X), r["X"], method="trf", jac="3-point", xtol=1e-15,
                                ftol=1e-15, gtol=1e-15)
            assert close(r["X"], sol.x), (i, j)
            n += 1
    assert n > 60


def test_rule_6_stopping_point_does_not_depend_on_the_last_bits_of_the_start():
    """Rule 6 takes a step only if c strictly decreases.  Judged by comparing c(X + d) with c(X) as two rounded float64
    sums, that cannot see a decrease under eps c, i.e. a step under ~1e-10, and whether the last useful step is taken
    then depends on the last bits of the start: moving the start by 1e-13 relative, the distance between two correct
    eigen-solvers, moves the final errors by ~1e-7 px (printed).  Judged by the difference formed from the step
    (robust_restated.cost_change, what the kernel does too) it moves them by ~2e-13, as five unconditional Gauss-Newton
    steps do.  Asserted: 1e-11 px, the 3e-14 px rounding of an error with a factor 300."""
    def refine_by_sums(P, kp, inl, X):
        w, c = np.ones(len(P)), rr.reprojection_cost(P, kp, np.ones(len(P)), inl, X)
        for _ in range(5):
            H, g = np.zeros((3, 3)), np.zeros(3)
            for v in inl:
                p = P[v] @ np.append(X, 1.0)
                Jm = (P[v, :2, :3] * p[2] - np.outer(p[:2], P[v, 2, :3])) / p[2] ** 2
                H, g = H + Jm.T @ Jm, g + Jm.T @ (p[:2] / p[2] - kp[v])
            Xn = X + np.linalg.solve(H, -g)
            c2 = rr.reprojection_cost(P, kp, w, inl, Xn)
            if not c2 < c:
                break
            X, c = Xn, c2
        return X

    worst, worst_sums = 0.0, 0.0
    for V, J in rc.SHAPES:
        c = rc.gross(V, J)
        res = run(c, inlier_px=rc.INLIER_PX, refine_iters=0)
        for i in range(6):
            P = step_P(c, i)
            for j in range(J):
                r, kp = res["joints"][i][j], f64(c["kp"][i, :, j])
                Xa = rr.refine(P, kp, np.ones(V), r["inliers"], r["X"], 5)[0]
                Xb = rr.refine(P, kp, np.ones(V), r["inliers"], r["X"] * (1 + 1e-13), 5)[0]
                worst = max(worst, float(np.abs(rr.errors(P, kp, Xa)[0] - rr.errors(P, kp, Xb)[0]).max()))
                Sa, Sb = refine_by_sums(P, kp, r["inliers"], r["X"]), refine_by_sums(P, kp, r["inliers"], r["X"] * (1 + 1e-13))
                worst_sums = max(worst_sums, float(np.abs(rr.errors(P, kp, Sa)[0] - rr.errors(P, kp, Sb)[0]).max()))
    print(f"largest change of a final error under a 1e-13 relative change of the start: {worst:.3e} px "
          f"(decrease judged by two rounded sums: {worst_sums:.3e} px)")
    assert worst < 1e-11


def test_cost_change_is_the_difference_of_the_costs():
    """cost_change against c(X + d) - c(X) in 50-digit arithmetic on steps from 1e-3 down to 1e-12, where the float64
    difference of the two sums has lost every digit"""
    from mpmath import mp, mpf
    mp.dps = 50
    c = rc.gross(8, 17)
    P, kp, inl = step_P(c, 0), f64(c["kp"][0, :, 0]), (1, 2, 4, 5, 7)
    X = rr.dlt(P, kp, inl)[0]

    def cost(Xm):
        tot = mpf(0)
        for v in inl:
            p = [sum(mpf(float(P[v, a, k])) * Xm[k] for k in range(3)) + mpf(float(P[v, a, 3])) for a in range(3)]
            tot += (p[0] / p[2] - mpf(float(kp[v, 0]))) ** 2 + (p[1] / p[2] - mpf(float(kp[v, 1]))) ** 2
        return tot

    rng = np.random.default_rng(0)
    for scale in (1e-3, 1e-6, 1e-9, 1e-12):
        d = rng.normal(size=3) * scale
        want = cost([mpf(float(X[k])) + mpf(float(d[k])) for k in range(3)]) - cost([mpf(float(X[k])) for k in range(3)])
        got = rr.cost_change(P, kp, np.ones(8), inl, X, d)
        assert abs(got - float(want)) <= 1e-9 * abs(float(want)), (scale, got, float(want))


# ---- the rules one by one ---------------------------------------------------------------------------------------------------
def test_rules_on_hand_built_cases():
    hb = rc.hand_built()
    c, uc, kw = hb["nan keypoint"]
    res = run(c, uc, **kw)
    r = res["joints"][0][2]
    assert not r["elig"][1] and np.isnan(res["err"][0, 1, 2]) and np.isfinite(res["err"][0, [0, 2, 3], 2]).all()
    assert not res["inlier_views"][0, 2] & 2 and res["ok"][0, 2] and len(r["hyps"]) == 3
    for j in (5, 6):                                   # no eligible view / one eligible view: the joint fails
        assert res["failed"][1, j] and not res["ok"][1, j] and res["inlier_views"][1, j] == 0
        assert np.isnan(res["joints3d"][1, j]).all() and np.isnan(res["err"][1, :, j]).all() and np.isnan(res["rms_px"][1, j])
    assert res["report"][1, 0] == res["ok"][1].sum() and res["report"][1, 1] == res["ok"][1].sum() / 8
    alive = ~res["failed"][1]
    for v in range(4):
        assert res["view_inlier_ratio"][1, v] == ((res["inlier_views"][1][alive] >> v) & 1).sum() / alive.sum()

    c, uc, kw = hb["low score"]
    res = run(c, uc, **kw)
    assert not res["joints"][0][3]["elig"][2] and np.isfinite(res["err"][0, 2, 3]) and not res["inlier_views"][0, 3] & 4
    assert res["failed"][0, 4] and np.isnan(res["err"][0, :, 4]).all()
    assert not res["joints"][1][0]["elig"][0] and res["ok"][1, 0]

    c, uc, kw = hb["view behind"]
    res = run(c, uc, **kw)
    assert not (res["inlier_views"][1] & 8).any() and res["ok"][1].all() and (res["err"][1, 3] > 10).all()
    assert res["view_inlier_ratio"][1, 3] == 0 and (res["inlier_views"][0] & 8).any()
    for r in res["joints"][1]:                         # a hypothesis of the turned view puts the point behind another camera
        assert all(len(h["inliers"]) < 2 for h in r["hyps"] if 3 in h["pair"])

    c, uc, kw = hb["two views"]
    res = run(c, uc, **kw)
    assert res["failed"][0, 1] and res["failed"][1, 2] and res["failed"].sum() == 2
    assert all(len(r["hyps"]) == 1 for row in res["joints"] for r in row)
    assert (res["inlier_views"][~res["failed"]] == 3).all()
    r3 = run(c, uc, min_inliers=2, refine_iters=0)
    P = step_P(c, 0)
    assert close(r3["joints3d"][0, 0], svd_dlt(P, f64(c["kp"][0, :, 0])))      # V = 2: the DLT, then the refinement

    c, uc, kw = hb["zero weights"]
    res = run(c, uc, **kw)
    plain = run(c, uc, conf_thr=-1.0, weighted=False)
    w = rr.weights(f64(c["conf"][0, :, 1]), True, 4)
    assert w[1] == 0 and rr.weights(f64(c["conf"][0, :, 2]), True, 4)[2] == 0 and rr.weights(f64(c["conf"][0, :, 3]), True, 4)[0] == 1
    assert res["joints"][0][1]["elig"].all()
    # a view of weight 0 is scored (it can be an inlier) but does not pull the fit
    r = res["joints"][0][1]
    others = tuple(v for v in r["inliers"] if v != 1)
    P, kp1 = step_P(c, 0), f64(c["kp"][0, :, 1])
    assert 1 in r["inliers"] and close(rr.refine(P, kp1, np.ones(4), others, rr.dlt(P, kp1, others)[0], 5)[0], r["X"])
    assert not close(r["X"], plain["joints3d"][0, 1], 1e-7)
    for j in (4, 5):                                   # no weight or one weight > 0: unweighted
        assert np.array_equal(res["joints3d"][1, j], plain["joints3d"][1, j])
    assert not np.array_equal(res["joints3d"][1, 0], plain["joints3d"][1, 0])


def test_min_inliers_reports_but_does_not_accept_a_joint_carried_by_two_views():
    c = rc.one_of_three()
    r2 = run(c, inlier_px=rc.INLIER_PX, min_inliers=2)
    r3 = run(c, inlier_px=rc.INLIER_PX, min_inliers=3)
    two = np.array([[bin(m).count("1") == 2 for m in row] for row in r2["inlier_views"]])
    assert two.any() and r2["ok"].all() and np.array_equal(r3["ok"], ~two)
    assert np.array_equal(r3["joints3d"], r2["joints3d"]) and np.array_equal(r3["rms_px"], r2["rms_px"])
    assert np.isnan(r3["joints3d_ok"][two]).all() and np.array_equal(r3["joints3d_ok"][~two], r3["joints3d"][~two])


# ---- what the stage is for ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,J", [(8, 17), (4, 12)])
def test_recovery_property(V, J):
    """0.5 px noise, 0 .. min(2, V - 3) views per joint moved by 25 .. 60 px, inlier_px = 3: the inlier set is exactly
    the unmoved views in every joint, and in every joint with a moved view the robust X is nearer to the X of the
    unmoved keypoints than the all-view DLT is.  No exception is allowed."""
    c = rc.gross(V, J)
    res = run(c, inlier_px=rc.INLIER_PX)
    clean = run({**c, "kp": c["clean"]}, inlier_px=rc.INLIER_PX)
    n_moved, worst, margin = 0, 0.0, np.inf
    for i in range(6):
        P = step_P(c, i)
        for j in range(J):
            want = sum(1 << v for v in range(V) if not c["moved"][i, v, j])
            assert res["inlier_views"][i, j] == want, (i, j)
            e = res["err"][i, :, j]
            margin = min(margin, float(np.abs(e - rc.INLIER_PX).min()))
            if c["moved"][i, :, j].any():
                n_moved += 1
                plain = rr.dlt(P, f64(c["kp"][i, :, j]), range(V))[0]
                d_rob = np.linalg.norm(res["joints3d"][i, j] - clean["joints3d"][i, j])
                assert d_rob < np.linalg.norm(plain - clean["joints3d"][i, j]), (i, j)
                worst = max(worst, float(d_rob))
    print(f"V={V} J={J}: {n_moved} joints with a moved view, robust X at most {worst * 1e3:.2f} mm from the unmoved keypoints' X, "
          f"smallest |final error - threshold| {margin:.2f} px")
    assert n_moved >= 30 and (clean["inlier_views"] == (1 << V) - 1).all()


# ---- the margins of every GPU case ---------------------------------------------------------------------------------------
def test_gpu_case_margins():
    """Conditions on the inputs under which two correct implementations give equal discrete outputs: no error of any
    scoring within 1e-6 px of inlier_px; no hypothesis with the winner's count and a cost within 1e-6 relative of the
    winner's that has another set; no score within 1e-6 of conf_thr (float32 rounding of a score near 0.3 is 3e-8); the
    eigenvalue ratio of every solved system under 1e6.  They do not depend on refine_iters or min_inliers."""
    seen = set()
    for name, c, use_conf, kw in rc.gpu_cases():
        key = (id(c), use_conf, kw.get("weighted", False), kw.get("conf_thr", 0.3), kw.get("inlier_px", 2.0))
        if key in seen:
            continue
        seen.add(key)
        res = run(c, use_conf, **kw)
        m = rr.margins(res, kw.get("inlier_px", 2.0))
        assert m["threshold"] > 1e-6 and not m["cost_tie"] and m["cond"] < 1e6, (name, m)
        if use_conf:
            d = np.abs(f64(c["conf"]) - kw.get("conf_thr", 0.3))
            assert np.nanmin(d) > 1e-6, name
    assert len(seen) >= 20
    c, steps = rc.big()                                # the T = 4096 launch is compared on these steps
    m = rr.margins(run(rc.take_steps(c, steps), inlier_px=rc.INLIER_PX), rc.INLIER_PX)
    assert m["threshold"] > 1e-6 and not m["cost_tie"] and m["cond"] < 1e6, m


# ---- the data-dependent branches, each forced by an input and asserted to have been taken --------------------------
def _branch_counts(res):
    n = dict(changed=0, changed_twice=0, fallback=0, gn_rejected=0, skipped=0, by_cost=0)
    for row in res["joints"]:
        for r in row:
            ch = sum(1 for rd in r["rounds"] if rd["changed"] and not rd["fallback"])
            n["changed"] += ch >= 1
            n["changed_twice"] += ch >= 2
            n["fallback"] += any(rd["fallback"] for rd in r["rounds"])
            n["gn_rejected"] += r["gn_rejected"]
            n["skipped"] += sum(h["skipped"] for h in r["hyps"])
            if r["winner"] is not None:
                wn = r["hyps"][r["winner"]]
                n["by_cost"] += any(not h["skipped"] and len(h["inliers"]) == len(wn["inliers"]) and h["inliers"] != wn["inliers"]
                                    for h in r["hyps"])
    return n


def test_branches_are_taken():
    """What was searched (seeds 100 V + J + 1000 k, k = 0 .. 3, on the restatement): moderate outliers (0 .. 3 views moved
    by 2 .. 7 px at inlier_px = 3) change the set in a refit in 10 - 19 of 102 joints at V = 8 and twice in 0 - 2; a refit
    that leaves fewer than two inliers did not occur unweighted and occurs at V = 3 with weighted refits (one view of
    two carries most of the weight, the other falls out); V = 3 with one grossly moved view gives winners that share
    their count with a hypothesis of another set."""
    n = _branch_counts(run(rc.moderate(8, 17), inlier_px=rc.INLIER_PX))
    assert n["changed"] >= 5 and n["changed_twice"] >= 1, n
    res = run(rc.moderate(3, 12), True, inlier_px=rc.INLIER_PX, weighted=True)
    n = _branch_counts(res)
    assert n["fallback"] >= 1, n
    for row in res["joints"]:                          # the fallback keeps the previous X and set: in round one the hypothesis'
        for r in row:
            if r["rounds"] and r["rounds"][0]["fallback"]:
                wn = r["hyps"][r["winner"]]
                assert r["inliers"] == wn["inliers"] and len(r["rounds"]) == 1
                P_unrefined = wn["X"]
                assert r["gn_taken"] > 0 or np.array_equal(r["X"], P_unrefined)
    n = _branch_counts(run(rc.one_of_three(), inlier_px=rc.INLIER_PX))
    assert n["by_cost"] >= 3, n
    c, uc, kw = rc.hand_built()["nan camera"]
    res = run(c, uc, **kw)
    n = _branch_counts(res)
    assert n["skipped"] == 7 * 17 and res["ok"].all(), n
    assert np.isnan(res["err"][1, 3]).all() and not (res["inlier_views"][1] & 8).any() and np.isfinite(res["err"][1, :3]).all()
    for j in range(17):                                # ... and the joints of that step are recovered from the other views
        want = sum(1 << v for v in range(8) if not c["moved"][1, v, j] and v != 3)
        assert res["inlier_views"][1, j] == want
    c, uc, kw = rc.hand_built()["refined to the end"]
    res = run(c, uc, **kw)
    # 32 steps: most joints go on taking steps of a few ulp; some reach a step that does not lower c (or that X cannot take)
    stopped = [(i, j) for i, row in enumerate(res["joints"]) for j, r in enumerate(row) if r["gn_rejected"]]
    assert stopped and all(res["joints"][i][j]["gn_taken"] < 32 for i, j in stopped), len(stopped)
    # ... and a rejected step from the start: refinement from where such a joint stopped takes no step
    for i, j in stopped:
        r = res["joints"][i][j]
        X, taken, rejected = rr.refine(step_P(c, i), f64(c["kp"][i, :, j]), np.ones(4), r["inliers"], r["X"], 5)
        assert taken == 0 and rejected and np.array_equal(X, r["X"])


# ---- the argument checks (these need the feature) -----------------------------------------------------------------------
def test_symbol_is_exported_and_rejects_bad_arguments_before_any_launch():
    lib = _lib.lib()
    assert "skimi_triangulate_robust" in _lib.exported_symbols()
    d = ctypes.c_void_p(16)

    def call(V=8, J=17, T=1, min_inliers=2, iters=5, px=2.0, first=d):
        return lib.skimi_triangulate_robust(first, d, d, d, None, 0.3, px, min_inliers, iters, 0, T, V, J, d, d, d, d, d, d, d, d, None)

    for kw, msg in ((dict(V=1), b"2..8 views"), (dict(V=9), b"2..8 views"), (dict(J=0), b"1..32 joints"), (dict(J=33), b"1..32 joints"),
                    (dict(T=0), b"steps > 0"), (dict(min_inliers=1), b"min_inliers"), (dict(min_inliers=9), b"min_inliers"),
                    (dict(V=3, min_inliers=4), b"min_inliers"), (dict(iters=-1), b"refine_iters"), (dict(iters=33), b"refine_iters"),
                    (dict(px=float("nan")), b"inlier_px"), (dict(first=None), b"null")):
        assert call(**kw) != 0, kw
        assert msg in lib.skimi_last_error(), (kw, lib.skimi_last_error())


def test_triangulate_robust_rejects_host_tensors_and_bad_shapes():
    def args(T=2, V=3, J=5):
        return torch.zeros(T, V, 3, 3), torch.zeros(T, V, 3, 3), torch.zeros(T, V, 3), torch.zeros(T, V, J, 2)

    with pytest.raises(_lib.SkimiError, match="device"):
        geometry.triangulate_robust(*args())
    with pytest.raises(_lib.SkimiError, match="device"):
        geometry.robust_launch(*args(), None, 0.3, 2.0, 2, 5, False)
    for shape in ((1, 17), (9, 17), (2, 33), (2, 0)):
        with pytest.raises(ValueError, match="views and 1..32 joints"):
            geometry.robust_launch(*args(V=shape[0], J=shape[1]), None, 0.3, 2.0, 2, 5, False)
    for bad in (1, 4, 0):
        with pytest.raises(ValueError, match="min_inliers"):
            geometry.robust_launch(*args(), None, 0.3, 2.0, bad, 5, False)
    for bad in (-1, 33):
        with pytest.raises(ValueError, match="refine_iters"):
            geometry.robust_launch(*args(), None, 0.3, 2.0, 2, bad, False)
    with pytest.raises(ValueError, match="inlier_px"):
        geometry.robust_launch(*args(), None, 0.3, float("nan"), 2, 5, False)
    with pytest.raises(ValueError, match="keypoints must be"):
        geometry.robust_launch(*args()[:3], torch.zeros(2, 3, 5), None, 0.3, 2.0, 2, 5, False)
    if torch.cuda.is_available():
        K, R, t, kp = (a.cuda() for a in args())
        with pytest.raises(ValueError, match="K must be contiguous float32"):
            geometry.robust_launch(K[:, :2], R, t, kp, None, 0.3, 2.0, 2, 5, False)
        with pytest.raises(ValueError, match="conf must be contiguous float32"):
            geometry.robust_launch(K, R, t, kp, torch.zeros(2, 3, 4).cuda(), 0.3, 2.0, 2, 5, False)
        with pytest.raises(_lib.SkimiError, match="device"):
            geometry.robust_launch(K, R, t, kp, torch.zeros(2, 3, 5), 0.3, 2.0, 2, 5, False)


def test_clip_path_rejects_bad_robust_arguments_before_any_launch():
    """the model is never called: None stands in for it"""
    T, S, J = 3, 2, 17
    frames = torch.zeros(T, S, 3, 28, 28)
    kp, scores = torch.zeros(T, S, J, 2), torch.zeros(T, S, J)
    with pytest.raises(ValueError, match="keypoints must be a device tensor"):
        infer.process_multi_view_clip(None, frames, kp, robust=True)
    with pytest.raises(ValueError, match="scores are only read by triage"):
        infer.process_multi_view_clip(None, frames, kp, scores=scores)
    for kw, msg in ((dict(min_inliers=1), "min_inliers"), (dict(min_inliers=3), "min_inliers"), (dict(refine_iters=33), "refine_iters"),
                    (dict(refine_iters=-1), "refine_iters"), (dict(inlier_px=float("nan")), "inlier_px")):
        with pytest.raises(ValueError, match=msg):
            infer.process_multi_view_clip(None, frames, kp, robust=True, **kw)
    for S_bad, J_bad in ((1, 17), (9, 17), (2, 33)):
        with pytest.raises(ValueError, match="robust=True needs 2..8 views and 1..32 joints"):
            infer.process_multi_view_clip(None, torch.zeros(T, S_bad, 3, 28, 28), torch.zeros(T, S_bad, J_bad, 2), robust=True)
    if torch.cuda.is_available():
        kd = kp.cuda()
        with pytest.raises(ValueError, match="scores must be a device tensor"):
            infer.process_multi_view_clip(None, frames, kd, scores=scores, robust=True)
        with pytest.raises(ValueError, match="keypoints must be a device tensor"):
            infer.process_multi_view_clip(None, frames, kd[:, :1], robust=True)
