"""CPU: what the device fusion / smoothing tests (tests/test_fuse_device_gpu.py) stand on.  fuse.savgol_operators is
fuse._savgol_interp as linear operators; and every case of tests/fuse_cases.py is STABLE: the host functions, which are
what the device is compared with, give the same NaN and branch patterns on inputs scaled by 1 + 1e-13 N(0, 1) and move
every compared output by no more than 1e-10, so a 1e-9 agreement is a statement about the kernels and not about the case."""
import numpy as np
import pytest

import fuse_cases as fc
from skiing_analysis_pytorch_amd import fuse


@pytest.mark.parametrize("win", [3, 5, 9])
@pytest.mark.parametrize("poly", [1, 2, 3])
def test_savgol_operators_reproduce_savgol_interp(win, poly):
    if poly >= win:
        with pytest.raises(ValueError):
            fuse.savgol_operators(win, poly)
        return
    fir, first, last = fuse.savgol_operators(win, poly)
    half = win // 2
    assert fir.shape == (win,) and first.shape == (half, win) and last.shape == (half, win)
    assert fir.dtype == first.dtype == last.dtype == np.float64
    rng = np.random.default_rng(win * 10 + poly)
    for n in (win, win + 1, win + 14):
        x = 10.0 * rng.normal(size=n) + 3.0
        y = np.empty(n)
        for k in range(half, n - half):
            y[k] = fir @ x[k - half:k + half + 1]
        y[:half] = first @ x[:win]
        y[n - half:] = last @ x[n - win:]
        want = fuse._savgol_interp(x, win, poly)
        assert np.max(np.abs(y - want) / (1.0 + np.abs(want))) <= 1e-12


def test_savgol_operators_refuse_bad_windows():
    for win, poly in ((4, 2), (0, 0), (-3, 1), (5, 5), (5, -1)):
        with pytest.raises(ValueError):
            fuse.savgol_operators(win, poly)
    fir, first, last = fuse.savgol_operators(1, 0)
    assert fir.tolist() == [1.0] and first.shape == (0, 1) and last.shape == (0, 1)
    assert [fuse.savgol_window(T) for T in (0, 1, 2, 8, 9, 500)] == [3, 3, 3, 7, 3, 9] and fuse.savgol_window(500, 4) == 5


def _stable(got, want):
    return fc.close(got, want, tol=1e-10)


@pytest.mark.parametrize("name", sorted(fc.h36m_cases()))
def test_h36m_cases_are_stable(name):
    c, h = fc.h36m_cases()[name], fc.host_h36m_case(name)
    rng = np.random.default_rng(7)
    left, right = fc.perturbed(rng, c["left"], c["right"])
    p = fc.host_h36m(left, right, c["kw"])
    assert np.array_equal(p["status"], h["status"])
    worst = max(_stable(p[k], h[k]) for k in ("fused", "R", "t", "s", "diag"))
    print(f"{name}: a 1e-13 perturbation moves the host outputs by {worst:.2e}")
    # no branch hangs on a hair: ||L - R|| against tau, the determinant against 0, the scales against 1e-8
    ok = h["status"]
    assert np.nanmin(np.abs(h["dist_tau"])) > 1e-6 and np.nanmin(np.abs(h["det"][ok])) > 0.5
    assert np.array_equal(p["det"][ok] < 0, h["det"][ok] < 0)
    for X in (c["left"], c["right"]):
        d = np.linalg.norm(X[:, 9] - X[:, 0], axis=1)
        assert np.nanmin(d) > 1e-2
    if name.startswith("T67_mixed"):
        # the special frames are what they are meant to be
        assert not ok[fc.F_NAN_PELVIS] and not ok[fc.F_TWO_TORSO] and ok.sum() == 65
        assert np.isnan(h["fused"][fc.F_NAN_PELVIS]).all() and h["det"][fc.F_MIRRORED] < 0 and (h["det"][ok] > 0).sum() > 50
        assert np.isfinite(h["fused"][fc.F_NAN_LEFT]).all() and np.isnan(h["fused"][fc.F_NAN_BOTH, 6]).all()
        assert np.isfinite(h["fused"][fc.F_NAN_TORSO]).all()        # the right joint is missing: the left one is taken
        sv = h["sv"][fc.F_PLANAR]
        assert 1e-5 < sv[2] / sv[0] < 1e-3, sv
        assert (h["dist_tau"][ok] > 0).any() and (h["dist_tau"][ok] < 0).any()      # both branches of fuse_two


@pytest.mark.parametrize("name", sorted(fc.views_cases()))
def test_views_cases_are_stable(name):
    c, h = fc.views_cases()[name], fc.host_views_case(name)
    rng = np.random.default_rng(8)
    p = fc.host_views(*fc.perturbed(rng, c["Xl"], c["Xr"], c["Ul"], c["Ur"]), c["kw"])
    assert np.array_equal(p["fit_ok"], h["fit_ok"])
    worst = max(_stable(p[k], h[k]) for k in fc.VIEW_FLOATS)
    print(f"{name}: a 1e-13 perturbation moves the host outputs by {worst:.2e}")
    fit = ~np.isnan(h["det"])
    assert np.abs(h["det"][fit]).min() > 0.5 and np.array_equal(p["det"][fit] < 0, h["det"][fit] < 0)
    # the canonical frames' scales and axes (thresholds 1e-9) and the fits' energies (1e-12) are far from their thresholds
    k = c["kw"]
    for X in (c["Xl"], c["Xr"]):
        hips = X[:, k["right_hip_idx"]] - X[:, k["left_hip_idx"]]
        up = 0.5 * (X[:, k["left_shoulder_idx"]] + X[:, k["right_shoulder_idx"]]) - 0.5 * (X[:, k["left_hip_idx"]] + X[:, k["right_hip_idx"]])
        assert np.nanmin(np.linalg.norm(hips, axis=1)) > 1e-3 and np.nanmin(np.linalg.norm(up, axis=1)) > 1e-3
        assert np.nanmin(np.linalg.norm(np.cross(hips, up), axis=1)) > 1e-6
        for t in range(X.shape[0]):
            rows = X[t][np.isfinite(X[t]).all(1)]
            assert len(rows) < 2 or ((rows - rows.mean(0)) ** 2).sum() > 1e-6
    if name == "J70_T65_mixed":
        assert not fit[fc.V_FEW_COMMON] and fit.sum() == 64
        assert np.array_equal(h["aligned"][fc.V_FEW_COMMON], c["Xr"][fc.V_FEW_COMMON])
        assert h["fit_ok"].sum() == 2 * 65 - 2 and not h["fit_ok"][fc.V_FEW_FIT, 0] and not h["fit_ok"][fc.V_FEW_COMMON, 0]
        assert (h["conf_x"][fc.V_NO_KEY] == 0).all() and (h["q_l"][fc.V_NO_KEY] == 0).all()
        assert np.isnan(h["err_l"][fc.V_NAN_2D, [2, 40, 68]]).all() and np.isnan(h["fused"][fc.V_NAN_3D, 17]).all()
        assert np.isfinite(h["fused"][fc.V_NAN_3D, [3, 30]]).all()
        assert (h["conf_l"][0] > 1e-3).any() and (h["conf_x"][0] > 1e-3).any()      # the confidences are not all underflow


def _savgol_combos():
    return [(T, v) for T in fc.SMOOTH_T for v in range(len(fc.SAVGOL_VARIANTS))
            if fuse.savgol_window(T, fc.SAVGOL_VARIANTS[v].get("win", 9)) > fc.SAVGOL_VARIANTS[v].get("poly", 2)]


@pytest.mark.parametrize("T", fc.SMOOTH_T)
def test_smoothing_cases_are_stable(T):
    X = fc.smooth_clip(T)
    rng = np.random.default_rng(9)
    (Xp,) = fc.perturbed(rng, X)
    for v in range(len(fc.EMA_VARIANTS)):
        _stable(fuse.temporal_smooth_ema(Xp, **fc.ema_kw(T, v)), fc.host_ema(T, v))
    for T_, v in _savgol_combos():
        if T_ == T:
            _stable(fuse.smooth_skeleton(Xp, **fc.SAVGOL_VARIANTS[v]), fc.host_savgol(T, v))
    if T >= 8:
        # the clip has what it is meant to have: a joint never seen, one that appears late, one that returns, and series
        # on both sides of the window
        ok = np.isfinite(X).all(axis=2)
        assert T >= 500 or not ok[:, 3].any() and not ok[0, 1] and ok[-1, 1] and not ok[3, 2] and ok[2, 2] and ok[5, 2]
        n = np.isfinite(X).sum(axis=0)
        win = fuse.savgol_window(T)
        assert (n >= win).any() and ((n > 0) & (n < win)).any()
        assert not np.array_equal(fc.host_savgol(T, 0), X, equal_nan=True)
