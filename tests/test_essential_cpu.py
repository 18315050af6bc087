"""CPU: the essential-matrix rules (DESIGN §2 "Essential matrix") on their NumPy restatement tests/essential_restated.py,
which tests/test_essential_gpu.py holds the kernels of csrc/essential.hip to.

Bounds, each from the restatement's own error (measured here, recorded in DESIGN):
  EPIPOLAR_BOUND 1e-11: |b^T E a| of a returned E on its own five points.  Cyclic Jacobi leaves the null vectors of the
      9 x 9 A^T A with ||A n|| of a few eps ||A||, and E is a combination of them with coefficients (x, y, z, 1) scaled
      to ||E||_F = sqrt 2; measured worst 2.1e-14 over the 500 samples, the prototype's 8.2e-13 before normalisation.
  RESIDUAL_BOUND (1e-10): the bound a candidate is kept under; measured worst after the polish 3.0e-16, before it 2.0e-9.
  AMONG_BOUND 5.9e-9: the true E among a noise-free sample's solutions, 10 x the restatement's worst (5.9e-10 in an entry of
      E over the 200 noise-free samples: a minimal sample's own conditioning).
  POSE_BOUND 9.0e-14: R, t^ and E of the noise-free cases against the rig's, 10 x the restatement's worst (9.0e-15, in R
      of clean_T8_step); tests/test_essential_gpu.py holds the kernel to the same figure.
  ROUTES_BOUND 1e-8: the two routes to the roots after the same polish; measured 5e-14."""
import numpy as np
import pytest

import essential_cases as ec
import essential_restated as er

EPIPOLAR_BOUND = 1e-11
AMONG_BOUND = 5.9e-9
POSE_BOUND = 9.0e-14
ROUTES_BOUND = 1e-8
STABLE = [c[0] for c in ec.comparison_cases()] + ["masked_T8_step"]


def _homog(x):
    return np.concatenate([x, np.ones(x.shape[:-1] + (1,))], axis=-1)


# ---- (a) the solver -----------------------------------------------------------------------------------------------------
def test_every_solution_meets_the_epipolar_and_the_cubic_constraints():
    a, b = ec.solver_samples()
    E, counts, d = ec.solver_restated()
    assert a.shape[0] >= 500 and counts.sum() > 4 * a.shape[0]
    valid = np.arange(10)[None] < counts[:, None]
    assert np.array_equal(np.isfinite(E).all(axis=(2, 3)), valid)
    epi = np.abs(np.einsum("spi,scij,spj->scp", _homog(b), E, _homog(a)))
    print("worst |b^T E a|", np.nanmax(epi))
    assert np.nanmax(epi) <= EPIPOLAR_BOUND
    assert np.allclose(np.sqrt((E[valid] ** 2).sum(axis=(1, 2))), np.sqrt(2.0), rtol=1e-14)
    # the ten constraints, evaluated on E itself: 2 E E^T E - tr(E E^T) E and det E, at ||E||_F = sqrt 2
    Ev = E[valid]
    EEt = Ev @ Ev.transpose(0, 2, 1)
    cubic = 2.0 * EEt @ Ev - np.trace(EEt, axis1=1, axis2=2)[:, None, None] * Ev
    worst = max(float(np.abs(cubic).max()), float(np.abs(np.linalg.det(Ev)).max()))
    print("worst constraint on E", worst, "kept under", er.RESIDUAL_BOUND)
    assert worst <= 2.0 ** 1.5 * er.RESIDUAL_BOUND          # ||E||^3 = 2^(3/2) times the residual at ||E|| = 1
    res = er.constraint_residual(d["M"], d["xyz"])
    assert np.nanmax(res) < er.RESIDUAL_BOUND
    x = d["xyz"][..., 0]
    assert (np.diff(x, axis=1)[valid[:, 1:]] >= 0).all()    # by x ascending


def test_eig_and_characteristic_polynomial_routes_give_the_same_solutions():
    a, b = ec.solver_samples()
    E, counts, _ = ec.solver_restated()
    E2, counts2 = er.five_point(a, b, roots=er.roots_charpoly)
    assert np.array_equal(counts, counts2)
    worst = np.nanmax(np.abs(E - E2))
    print("routes differ by", worst)
    assert worst <= ROUTES_BOUND


def test_one_more_polish_step_changes_nothing_beyond_rounding():
    a, b = ec.solver_samples()
    E, counts, _ = ec.solver_restated()
    E2, counts2 = er.five_point(a, b, steps=er.POLISH_STEPS + 1)
    assert np.array_equal(counts, counts2)
    diff = np.abs(E - E2)[np.isfinite(E)]
    print("one more step: worst", diff.max(), "median", np.median(diff))
    assert diff.max() <= 1e-14      # rule 4's criterion for the step count (measured 8.4e-15, median 5e-19)


# ---- (b) noise-free ---------------------------------------------------------------------------------------------------------
def test_the_true_E_is_among_the_solutions_of_every_noise_free_sample():
    import resect_cases as rc
    p = ec.pair(rc.rig(T=64, V=3, seed=71), 0, 2)          # the rig of solver_samples' first 200
    Et = er.skew(p["t"]) @ p["R"]
    E, counts, _ = ec.solver_restated()
    E = E[:200]
    dist = np.minimum(np.abs(E - Et).max(axis=(2, 3)), np.abs(E + Et).max(axis=(2, 3)))
    worst = np.nanmin(dist, axis=1).max()
    print("true E among the solutions to", worst)
    assert worst <= AMONG_BOUND


@pytest.mark.parametrize("name", [c[0] for c in ec.clean_cases()])
def test_noise_free_pose_is_the_rigs(name):
    _, p, kw = ec.case(name)
    r = ec.restated(name)
    assert r["success"].all() and (r["n_inliers"] == r["n_used"]).all() and (r["n_pose"] == r["n_used"]).all()
    eR, et = np.abs(r["R"] - p["R"]).max(), np.abs(r["t"] - p["t"]).max()
    eE = np.abs(r["E"] - er.skew(p["t"]) @ p["R"]).max()
    print(name, "R", eR, "t", et, "E", eE)
    assert max(eR, et, eE) <= POSE_BOUND


# ---- (c) ----------------------------------------------------------------------------------------------------------------------
def test_outlier_clip_keeps_most_of_the_true_inliers():
    name = "out10_T64_clip"
    _, p, kw = ec.case(name)
    assert kw["hypotheses"] == 300
    r = ec.restated(name)
    d = r["details"][0]
    true_inl, _, _ = er.score(er.skew(p["t"]) @ p["R"], d["a"], d["b"], d["tau"])
    rot = ec.rotation_angle_deg(r["R"][0], p["R"])
    print("winner", r["n_inliers"][0], "of the true E's", true_inl.sum(), "rotation error", rot, "deg, t",
          ec.direction_angle_deg(r["t"][0], p["t"]), "deg")
    assert r["n_inliers"][0] >= 0.8 * true_inl.sum()
    assert rot < 2.0


# ---- (d) stability of every comparison case -----------------------------------------------------------------------------------
def _problem(name):
    return ec.masked_case()[1:3] if name == "masked_T8_step" else ec.case(name)[1:]


def _groups(name, r):
    skip = (ec.MASKED_FAILED, ec.MASKED_FIVE) if name == "masked_T8_step" else ()
    return [g for g in range(len(r["n_used"])) if g not in skip]


def instabilities(p, kw, r, groups, dmax=50.0):
    """the conditions under which kernel and restatement must agree through `winner` -> (violations, pose movement)"""
    bad = []
    for g in groups:
        d = r["details"][g]
        # the winner leads the runner-up by an inlier or by more than 1e-6 relative in cost
        n2, c2 = d["runner"]
        if not (r["n_inliers"][g] > n2 or c2 - r["cost"][g] > 1e-6 * r["cost"][g]):
            bad.append((g, "runner-up"))
        # no point's e^2 within 1e-6 relative of tau^2
        t2 = d["tau"] ** 2
        if not (np.abs(d["e2"] - t2) > 1e-6 * t2).all():
            bad.append((g, "threshold"))
        # no inlier's depth within 1e-6 relative of 0 or distance_thresh, for any of the four candidates
        z = d["z"]
        if not (np.isfinite(z).all() and (np.abs(z) > 1e-6).all() and (np.abs(z - dmax) > 1e-6 * dmax).all()):
            bad.append((g, "depth"))
    # moving the keypoints by 1e-13 relative moves E, R, t by at most 1e-10
    rng = np.random.default_rng(5)
    x2 = p["x2d"] * (1.0 + 1e-13 * rng.standard_normal(p["x2d"].shape))
    r2 = er.essential_ransac(x2, p["K"], conf=p["conf"], **kw)
    moved = max(float(np.abs(r2[k][groups] - r[k][groups]).max()) for k in ("E", "R", "t"))
    if not moved <= 1e-10:
        bad.append(("all", "perturbation"))
    return bad, moved


@pytest.mark.parametrize("name", STABLE)
def test_comparison_case_is_stable(name):
    """a case that fails a condition gets another seed in essential_cases; none is dropped"""
    p, kw = _problem(name)
    r = ec.restated(name)
    bad, moved = instabilities(p, kw, r, _groups(name, r))
    print(name, "a 1e-13 perturbation moves the pose by", moved)
    assert not bad, (name, bad)


def test_masked_case_counts_and_the_failed_group():
    name, p, kw, n_used = ec.masked_case()
    r = ec.restated(name)
    assert np.array_equal(r["n_used"], n_used)
    g = ec.MASKED_FAILED
    assert r["success"][g] == 0 and np.isnan(r["R"][g]).all() and np.isnan(r["t"][g]).all() and np.isnan(r["E"][g]).all()
    assert np.isnan(r["cost"][g]) and r["n_inliers"][g] == 0 and r["n_pose"][g] == 0 and tuple(r["winner"][g]) == (-1, -1)
    assert not r["inliers"][g * ec.J:(g + 1) * ec.J].any() and not r["pose_mask"][g * ec.J:(g + 1) * ec.J].any()
    g = ec.MASKED_FIVE                                 # exactly five points: every sample is those five, and fits them
    assert r["success"][g] == 1 and r["n_inliers"][g] == 5 and r["cost"][g] <= 1e-20
    used = er.mask(p["x2d"], p["conf"], kw["min_conf"])
    assert np.array_equal(r["inliers"].astype(bool) & ~used, np.zeros_like(used))


# ---- (e) the sampling stream ------------------------------------------------------------------------------------------------
def test_splitmix64_known_values():
    # the published test vector of splitmix64 from state 0 (Vigna's splitmix64.c; also java.util.SplittableRandom)
    s, out = 0, []
    for _ in range(3):
        s, z = er.splitmix64(s)
        out.append(z)
    assert out == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]


@pytest.mark.parametrize("seed, g, h, m, want", [
    (0, 0, 0, 5, [0, 4, 2, 3, 1]), (0, 0, 0, 17, [12, 9, 2, 14, 7]), (0, 0, 0, 1088, [692, 655, 172, 1051, 874]),
    (0x123456789ABCDEF, 3, 7, 5, [3, 0, 2, 4, 1]), (0x123456789ABCDEF, 3, 7, 17, [8, 16, 12, 15, 1]), (0x123456789ABCDEF, 3, 7, 1088, [127, 229, 832, 233, 372]),
])
def test_sampling_stream(seed, g, h, m, want):
    """`want` was worked out apart from the restatement, in wrapping 64-bit integers from rule 3's text; for seed 0 the
    draws are the published vector's second to sixth outputs mod m (the first is discarded)"""
    assert er.draw_sample(seed, g, h, m) == want
