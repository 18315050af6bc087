"""GPU: the camera calibration (csrc/calibrate.hip: calibrate_kernel; geometry.calibrate_camera, calibration.calibrate_camera,
calibration.leave_one_out) against the float64 restatement tests/calibrate_restated.py on the inputs of
tests/calibrate_cases.py.

Bounds (tests/test_calibrate_cpu.py: MOVED, bound): counts, success and NaN patterns equal; an output whose stopping point
moves by under 1e-10 when the start moves by 1e-13 relative is held to 1e-9 (1 + |x|), the project's float64 tolerance; the
others to ten times the restatement's own measured movement.  With the rational model the coefficients are not determined
by the data, so those cases compare the invariants only: costs, rms, err, the per-view statistics and the distortion map's
pixel displacement on a 25 x 15 grid over the frame."""
import numpy as np
import pytest
import torch

import calibrate_cases as cc
import calibrate_restated as cr
from skiing_analysis_pytorch_amd import _lib, calibration, geometry
from test_calibrate_cpu import ALL_KEYS, INVARIANT_KEYS, bound

dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
ALL = cc.cases()
NAMES = cr.NAMES


def kernel(d, kw, **over):
    kw = dict(kw, **over)
    mask = kw.pop("mask")
    free = tuple(k for i, k in enumerate(NAMES) if (mask >> i) & 1)
    kw = {k: (dev(v) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    r = geometry.calibrate_camera(dev(d["obj"]), dev(d["img"]), cc.SIZE, free=free, **kw)
    assert r.success.dtype == torch.bool and r.n_evals.dtype == torch.int32 and r.K.dtype == torch.float64
    out = {k: getattr(r, k).cpu().numpy() for k in r._fields}
    out["view_stats"] = np.stack([out["mean_err"], out["rms_err"], out["max_err"]], -1)
    return out


_WANT = {}


def restated(name):
    """the restatement's result of a case, computed once"""
    if name not in _WANT:
        _, d, kw = next(x for x in ALL if x[0] == name)
        _WANT[name] = cc.run(d, kw)
    return _WANT[name]


def _close(got, want, tol, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    diff = np.abs(got - want) / (1 + np.abs(want))
    worst = float(np.nanmax(diff, initial=0.0))
    assert worst <= tol, (what, worst, tol)
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("case", ALL, ids=lambda c: c[0])
def test_kernel_matches_restatement(case):
    name, d, kw = case
    got, want = kernel(d, kw), restated(name)
    for k in ("n_views", "n_corners"):
        assert np.array_equal(got[k], want[k]), (name, k)
    assert np.array_equal(got["success"], want["success"].astype(bool)), name
    assert np.array_equal(got["n_evals"] == 0, want["n_evals"] == 0), name
    worst = {k: _close(got[k], want[k], bound(name, k), f"{name}: {k}") for k in (INVARIANT_KEYS if d["rational"] else ALL_KEYS)}
    ok = np.isfinite(want["rms"])
    assert np.isnan(got["K"][~ok]).all() and np.isnan(got["dist"][~ok]).all() and np.isnan(got["std"][~ok]).all()
    for g in np.flatnonzero(ok):
        m = np.abs(cc.distortion_map_px(got["K"][g], got["dist"][g]) - cc.distortion_map_px(want["K"][g], want["dist"][g])).max()
        worst["map"] = max(worst.get("map", 0.0), float(m))
    assert worst.get("map", 0.0) <= bound(name, "map"), (name, worst["map"])
    print(name, {k: f"{v:.1e}" for k, v in worst.items()}, "n_evals", got["n_evals"], want["n_evals"])


@pytest.mark.gpu
def test_a_group_is_bitwise_what_it_is_alone_in_a_batch_and_on_a_rerun():
    name, d, kw = next(x for x in ALL if x[0] == "V8_c5_G5")
    full, again = kernel(d, kw), kernel(d, kw)
    for k in full:
        assert np.array_equal(full[k], again[k], equal_nan=True), (k, "rerun")
    for g in range(5):
        alone = kernel(d, kw, use=kw["use"][g:g + 1])
        for k in full:
            assert np.array_equal(alone[k][0], full[k][g], equal_nan=True), (g, k)
    # the failed group (2 views) is NaN with zero evaluations, and its counts are still reported
    assert full["n_evals"][4] == 0 and not full["success"][4] and full["n_views"][4] == 2
    for k in ("K", "dist", "R", "t", "rvec", "err", "rms", "cost0", "cost", "std"):
        assert np.isnan(full[k][4]).all(), k
    # an unused view of a good group: NaN pose and errors
    assert np.isnan(full["R"][1, 3]).all() and np.isnan(full["err"][1, 3]).all() and np.isfinite(full["R"][1, 2]).all()


@pytest.mark.gpu
def test_fixed_parameters_keep_their_start_and_have_no_std():
    name, d, kw = next(x for x in ALL if x[0] == "V6_c5_fixed_pp")
    got = kernel(d, kw)
    assert got["K"][0, 0, 2] == (cc.SIZE[0] - 1) / 2 and got["K"][0, 1, 2] == (cc.SIZE[1] - 1) / 2
    assert np.isnan(got["std"][0, [2, 3, 9, 10, 11]]).all() and np.isfinite(got["std"][0, [0, 1, 4, 5, 6, 7, 8]]).all()
    assert (got["dist"][0, 5:] == 0).all()
    name, d, kw = next(x for x in ALL if x[0] == "V6_c5_zero_tangent")
    got = kernel(d, kw)
    assert (got["dist"][0, 2:4] == 0).all() and np.isnan(got["std"][0, 6:8]).all()


@pytest.mark.gpu
def test_bad_arguments_return_an_error_code_without_a_launch():
    lib = _lib.lib()
    _, d, kw = ALL[0]
    V, n = d["img"].shape[:2]
    obj, img = dev(d["obj"]), dev(d["img"])
    f64 = lambda *s: torch.full(s, 7.0, dtype=torch.float64, device="cuda")    # noqa: E731
    i32 = lambda *s: torch.full(s, 7, dtype=torch.int32, device="cuda")        # noqa: E731
    # K, dist, R, t, rvec, err, view_stats, rms, cost0, cost, std, n_evals, n_views, n_corners, success
    outs = [f64(1, 3, 3), f64(1, 12), f64(1, V, 3, 3), f64(1, V, 3), f64(1, V, 3), f64(1, V, n), f64(1, V, 3), f64(1), f64(1), f64(1),
            f64(1, 12), i32(1), i32(1), i32(1), i32(1)]
    nws = lib.skimi_calibrate_workspace_bytes(1, V, n)
    assert nws > 0 and lib.skimi_calibrate_workspace_bytes(1, 1025, n) == 0 and lib.skimi_calibrate_workspace_bytes(1, V, 3) == 0
    assert lib.skimi_calibrate_workspace_bytes(0, V, n) == 0 and lib.skimi_calibrate_workspace_bytes(1, V, 4097) == 0
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda")

    def call(obj=obj, img=img, G=1, V=V, n=n, width=1920, height=1080, mask=kw["mask"], max_evals=200, outs=outs, ws=ws, ws_bytes=nws):
        p = [None if o is None else o.data_ptr() for o in outs]
        return lib.skimi_calibrate_camera(_lib.ptr(obj), _lib.ptr(img), None, None, None, G, V, n, width, height, mask, max_evals, *p,
                                          _lib.ptr(ws), ws_bytes, None)

    for bad, msg in ((dict(obj=None), b"NULL input"), (dict(img=None), b"NULL input"), (dict(outs=[None] + outs[1:]), b"NULL output"),
                     (dict(outs=outs[:-1] + [None]), b"NULL output"), (dict(G=0), b"G ="), (dict(V=0), b"views"), (dict(V=1025), b"views"),
                     (dict(n=3), b"corners"), (dict(n=4097), b"corners"), (dict(width=0), b"image size"), (dict(height=-1), b"image size"),
                     (dict(mask=-1), b"free_mask"), (dict(mask=1 << 12), b"free_mask"), (dict(max_evals=0), b"max_evals"),
                     (dict(ws=None), b"workspace"), (dict(ws_bytes=nws - 8), b"workspace")):
        assert call(**bad) == -1, bad                      # SKIMI_ERR_ARG
        assert msg in lib.skimi_last_error(), (bad, lib.skimi_last_error())
    torch.cuda.synchronize()
    for o in outs:                                         # nothing was launched: the outputs are untouched
        assert bool((o == 7).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert int(outs[12][0]) == V and int(outs[13][0]) == V * n and int(outs[14][0]) == 1 and 1 < int(outs[11][0]) < 200
    with pytest.raises(_lib.SkimiError, match="device tensors"):
        geometry.calibrate_camera(torch.from_numpy(d["obj"]), img, cc.SIZE)
    with pytest.raises(ValueError):
        geometry.calibrate_camera(obj, img[:, :-1], cc.SIZE)
    with pytest.raises(ValueError, match="unknown parameter"):
        geometry.calibrate_camera(obj, img, cc.SIZE, free=("fx", "k7"))


@pytest.mark.gpu
def test_calibrate_camera_end_to_end_prunes_the_shifted_view():
    """calibration.calibrate_camera on the V = 24 fixture (5 coefficients) with view 11's corners shifted by 3 px: its mean
    error is the largest, prune_top_ratio = 1 / 24 puts the 23/24 quantile just under it, the prune step drops exactly that
    view, and the rms falls"""
    _, d, _ = cc.case("V24_prune", 24, 5, 0.1, 21)
    img = d["img"].copy()
    img[11] += np.array([3.0, -3.0]) / np.sqrt(2.0) * np.where(np.arange(img.shape[1]) % 2 == 0, 1.0, -1.0)[:, None]
    cfg = calibration.CalibConfig(rational_model=False, prune_top_ratio=1.0 / 24)
    names = [f"view_{v:02d}" for v in range(24)]
    res = calibration.calibrate_camera(img, cfg, image_size=cc.SIZE, names=names)
    assert res["status"] == "Success" and res["dropped_names"] == ["view_11"] and res["num_images"] == 23
    assert res["used_names"] == [k for k in names if k != "view_11"]
    first = cr.calibrate_camera(d["obj"], img, cc.SIZE, mask=cr.free_mask(rational_model=False))
    use = np.ones((1, 24), np.uint8)
    use[0, 11] = 0
    second = cr.calibrate_camera(d["obj"], img, cc.SIZE, use=use, mask=cr.free_mask(rational_model=False))
    assert second["rms"][0] < first["rms"][0]
    assert abs(res["rms_reproj_error"] - second["rms"][0]) <= 1e-9 * (1 + second["rms"][0])
    assert abs(res["rms_before_prune"] - first["rms"][0]) <= 1e-9 * (1 + first["rms"][0])
    assert np.abs(res["camera_matrix"] - second["K"][0]).max() <= 1e-6 * (1 + np.abs(second["K"][0]).max())
    for k in ("global_mean_px", "global_median_px", "global_p95_px", "coverage_ratio", "edge_points_ratio", "hfov_deg", "fx",
              "straightness_rms_before_px", "straightness_rms_after_px", "std_intrinsics", "rvecs", "tvecs", "per_image"):
        assert k in res, k
    assert len(res["per_image"]) == 23 and res["straightness_rms_after_px"] < res["straightness_rms_before_px"]
    # prune disabled: nothing is dropped
    res0 = calibration.calibrate_camera(img, calibration.CalibConfig(rational_model=False, prune_top_ratio=0.0), image_size=cc.SIZE)
    assert res0["dropped_names"] == [] and res0["num_images"] == 24


@pytest.mark.gpu
def test_leave_one_out_equals_single_calls_bitwise():
    _, d, kw = next(x for x in ALL if x[0] == "V8_c5_n0.1")
    cfg = calibration.CalibConfig(rational_model=False, prune_top_ratio=0.0)
    loo = calibration.leave_one_out(d["img"], cfg, image_size=cc.SIZE)
    V = d["img"].shape[0]
    assert loo["K"].shape == (V, 3, 3) and loo["dist"].shape == (V, 12) and loo["rms"].shape == (V,)
    for v in range(V):
        use = np.ones((1, V), np.uint8)
        use[0, v] = 0
        one = kernel(d, kw, use=use)
        assert np.array_equal(loo["K"][v], one["K"][0]) and np.array_equal(loo["dist"][v], one["dist"][0]), v
        assert loo["rms"][v] == one["rms"][0]
    p = np.concatenate([loo["K"][:, [0, 1, 0, 1], [0, 1, 2, 2]], loo["dist"][:, :8]], 1)
    assert np.array_equal(loo["spread"]["std"], p.std(axis=0)) and np.array_equal(loo["spread"]["max"], p.max(axis=0))
    assert loo["spread"]["names"] == list(geometry.CALIB_PARAMS)
