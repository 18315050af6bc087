"""GPU: the chessboard detector (csrc/chessboard.hip: chess_response_kernel, chess_count_kernel, chess_write_kernel,
corner_subpix_kernel; geometry.chessboard_candidates, geometry.corner_subpix, calibration.find_chessboard_corners,
calibration.calibrate_from_frames) against the restatement tests/chessboard_restated.py on the frames of
tests/chessboard_cases.py.

Bounds: the candidate stage is integer, so xy, response, count and rmax are bitwise equal.  The refinement is float64 with
the same per-element expressions and a different order of its five window sums: 1e-9 px, the project's bound for float64
kernels whose summation order differs, with ok equal; two runs are bitwise identical.  The truth's bound
(chessboard_cases.TRUTH_BOUND_PX) is asked of the end-to-end result only."""
import functools

import numpy as np
import pytest
import torch

import chessboard_cases as cb
import chessboard_restated as cs
from skiing_analysis_pytorch_amd import calibration, geometry

dev = lambda a: torch.from_numpy(np.array(a)).cuda()   # noqa: E731  (a copy: the cached frames are read-only)
FIELDS = ("xy", "response", "count", "rmax")
SUBPIX_TOL = 1e-9


@functools.lru_cache(maxsize=None)
def frame(name):
    """the named test frames, uint8 [H, W, ch]"""
    if name.startswith("view"):                       # view<k>_ch<c>
        v, ch = name[4:].split("_ch")
        return cb.channels(cb.render(int(v)), int(ch))
    if name == "crop":                                # 637 x 353: ragged tile edges, odd row length
        return cb.channels(cb.render(13)[3:356, 2:639], 3)
    if name == "half_out":
        return cb.channels(cb.render(0, cb.HALF_OUT_SHIFT), 1)
    if name == "constant":
        return np.full((70, 150, 3), 90, np.uint8)
    if name == "noise":
        return cb.noise_frame()
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def want_candidates(name, max_candidates=1024):
    return cs.candidates(frame(name), max_candidates=max_candidates)


def got_candidates(frames, **kw):
    r = geometry.chessboard_candidates(dev(frames), **kw)
    assert all(getattr(r, k).dtype == torch.int32 for k in FIELDS)
    return {k: getattr(r, k).cpu().numpy() for k in FIELDS}


def same(got, want, what):
    for k in FIELDS:
        assert np.array_equal(got[k], want[k]), (what, k, got["count"], want["count"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["view0_ch1", "view0_ch3", "view0_ch4", "crop", "half_out", "constant"])
def test_candidates_are_bitwise_the_restatement(name):
    got = got_candidates(frame(name)[None])
    want = want_candidates(name)
    assert got["xy"].shape == (1, 1024, 2) and got["count"].shape == (1,)
    same({k: v[0] for k, v in got.items()}, want, name)
    if name == "constant":
        assert got["count"][0] == 0 and got["rmax"][0] == 0
    print(name, "count", got["count"][0], "rmax", got["rmax"][0])


@pytest.mark.gpu
def test_candidates_overflow_keeps_the_first_in_pixel_order():
    got = got_candidates(frame("noise")[None], max_candidates=64)
    want = want_candidates("noise", 64)
    assert got["count"][0] > 64 and (got["xy"][0] >= 0).all()
    same({k: v[0] for k, v in got.items()}, want, "noise")


@pytest.mark.gpu
def test_candidates_of_a_view_into_a_clip_whose_frames_start_at_odd_addresses():
    """frames[1:] of a 637 x 353 x 3 clip starts 674583 bytes into its allocation: the rows' aligned dword loads begin inside
    the frame before it, and nothing of that frame may show"""
    clip = dev(np.stack([frame("noise")[:1, :1].repeat(353, 0).repeat(637, 1), frame("crop"), frame("crop")[::-1]]))
    r = geometry.chessboard_candidates(clip[1:])
    assert clip[1:].data_ptr() % 4 == 3
    same({k: getattr(r, k).cpu().numpy()[0] for k in FIELDS}, want_candidates("crop"), "sliced clip")
    pts = r.xy[:, :54].double()
    got = geometry.corner_subpix(clip[1:], pts, win=cb.WIN)
    want, want_ok = cs.corner_subpix(frame("crop"), pts[0].cpu().numpy(), win=cb.WIN)
    assert np.array_equal(got.ok.cpu().numpy()[0], want_ok)
    close(got.points.cpu().numpy()[0], want, "sliced clip")


@pytest.mark.gpu
def test_subpix_before_it_has_converged():
    """two rounds: the points are still moving, so the window sums' order shows in the last bits"""
    frames, pts = subpix_inputs(cb.WIN)
    r = geometry.corner_subpix(dev(frames), dev(pts), win=cb.WIN, iters=2)
    want = [cs.corner_subpix(f, p, win=cb.WIN, iters=2) for f, p in zip(frames, pts)]
    assert np.array_equal(r.ok.cpu().numpy(), np.stack([w[1] for w in want]))
    close(r.points.cpu().numpy(), np.stack([w[0] for w in want]), "2 rounds")
    zero = geometry.corner_subpix(dev(frames), dev(pts), win=cb.WIN, iters=0)
    assert np.array_equal(zero.points.cpu().numpy(), pts, equal_nan=True)


@pytest.mark.gpu
def test_candidates_five_axes_and_a_frame_alone():
    names = ["view0_ch1", "view9_ch1", "view13_ch1", "half_out"]
    clip = np.stack([frame(n) for n in names]).reshape(2, 2, 360, 640, 1)
    got = got_candidates(clip)
    assert got["xy"].shape == (2, 2, 1024, 2) and got["rmax"].shape == (2, 2)
    for i, n in enumerate(names):
        same({k: v[i // 2, i % 2] for k, v in got.items()}, want_candidates(n), n)
    pair = got_candidates(clip.reshape(4, 360, 640, 1)[[1, 3]])
    for j, i in enumerate((1, 3)):
        alone = got_candidates(frame(names[i])[None])
        for k in FIELDS:
            assert np.array_equal(pair[k][j], alone[k][0]) and np.array_equal(pair[k][j], got[k][i // 2, i % 2]), (names[i], k)


def subpix_inputs(win):
    """frames [3, H, W, 1] and points [3, M, 2]: each view's restated candidates, then the special starts"""
    frames = np.stack([frame(f"view{v}_ch1") for v in cb.VIEWS])
    rows = []
    for v in cb.VIEWS:
        c = want_candidates(f"view{v}_ch1")
        special = [cb.FLAT_POINT, list(cb.far_point(v, win)), [np.nan, 3.0], [-0.5, 4.0], [640.0, 10.0], [639.75, 359.75]]
        rows.append(np.concatenate([c["xy"][:54].astype(np.float64), special]))
    return frames, np.stack(rows)


@functools.lru_cache(maxsize=None)
def want_subpix(win):
    frames, pts = subpix_inputs(win)
    out = [cs.corner_subpix(f, p, win=win) for f, p in zip(frames, pts)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def close(got, want, what):
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    worst = float(np.nanmax(np.abs(got - want), initial=0.0))
    print(what, f"worst {worst:.2e} px")
    assert worst <= SUBPIX_TOL, (what, worst)


@pytest.mark.gpu
@pytest.mark.parametrize("win", [(5, 5), (11, 11), (4, 7)])
def test_subpix_matches_the_restatement(win):
    frames, pts = subpix_inputs(win)
    r = geometry.corner_subpix(dev(frames), dev(pts), win=win)
    again = geometry.corner_subpix(dev(frames), dev(pts), win=win)
    assert r.points.dtype == torch.float64 and r.ok.dtype == torch.bool and r.points.shape == pts.shape
    got, ok = r.points.cpu().numpy(), r.ok.cpu().numpy()
    assert np.array_equal(got, again.points.cpu().numpy(), equal_nan=True) and np.array_equal(ok, again.ok.cpu().numpy())
    want, want_ok = want_subpix(win)
    assert np.array_equal(ok, want_ok), (win, np.argwhere(ok != want_ok))
    close(got, want, f"win {win}")
    flat, far = 54, 55
    assert ok[:, flat].all() and np.array_equal(got[:, flat], pts[:, flat])           # singular system: unchanged
    runs_off = [2] if win == (11, 11) else [0, 1, 2]                                  # chessboard_cases.far_point
    assert not ok[runs_off, far].any() and np.array_equal(got[runs_off, far], pts[runs_off, far])      # reverted
    assert not ok[:, 56:59].any()                                                     # not finite / outside the frame


@pytest.mark.gpu
def test_subpix_border_colour_and_count():
    crop, start, _ = cb.border_case()
    f3 = cb.channels(crop, 3)
    pts = np.array([start, [3.0, 3.0], start])
    for fr in (crop[..., None], f3, cb.channels(crop, 4)):
        r = geometry.corner_subpix(dev(fr[None]), dev(pts[None]), count=dev(np.array([2], np.int32)), win=cb.WIN)
        want, want_ok = cs.corner_subpix(fr, pts, count=2, win=cb.WIN)
        assert np.array_equal(r.ok.cpu().numpy()[0], want_ok) and want_ok.tolist() == [True, True, False]
        close(r.points.cpu().numpy()[0], want, f"border, ch {fr.shape[-1]}")
    # integer points and five axes
    xy = want_candidates("view0_ch1")["xy"][:54]
    r = geometry.corner_subpix(dev(frame("view0_ch1")[None, None]), dev(xy[None, None]), win=cb.WIN)
    want, want_ok = cs.corner_subpix(frame("view0_ch1"), xy, win=cb.WIN)
    assert r.points.shape == (1, 1, 54, 2) and np.array_equal(r.ok.cpu().numpy()[0, 0], want_ok)
    close(r.points.cpu().numpy()[0, 0], want, "int32 points")


@pytest.mark.gpu
def test_find_chessboard_corners_end_to_end():
    frames = np.stack([frame(f"view{v}_ch1") for v in cb.VIEWS] + [frame("half_out")])
    corners, found = calibration.find_chessboard_corners(dev(frames), cb.BOARD, win=cb.WIN)
    assert corners.shape == (4, 54, 2) and found.tolist() == [True, True, True, False]
    assert np.isnan(corners[3]).all()
    for i, v in enumerate(cb.VIEWS):
        truth = cb.canonical(cb.truth(v))
        err = np.hypot(*(corners[i] - truth).T)
        print(f"view {v}: mean {err.mean():.3f} px, worst {err.max():.3f} px")
        assert err.max() <= cb.TRUTH_BOUND_PX, (v, err.max())                # the truth's order, every corner
        close(corners[i], cb.restated(v)[0], f"view {v} against the restatement")


@pytest.mark.gpu
def test_calibrate_from_frames_is_calibrate_camera_on_the_detected_corners():
    frames = dev(np.stack([frame(f"view{v}_ch1") for v in cb.CALIB_VIEWS] + [np.full((360, 640, 1), 90, np.uint8)]))
    cfg = calibration.CalibConfig(max_evals=60)
    names = [f"board_{v}" for v in cb.CALIB_VIEWS] + ["empty"]
    got = calibration.calibrate_from_frames(frames, cfg, names=names, win=cb.WIN)
    corners, found = calibration.find_chessboard_corners(frames, cfg.board_size, win=cb.WIN)
    assert found.tolist() == [True] * 6 + [False]
    want = calibration.calibrate_camera(corners[found], cfg, image_size=cb.SIZE, names=names[:6])
    assert got["status"] == "Success" and got["num_detected"] == 6 and got["used_names"] == names[:6] and got["image_size"] == cb.SIZE
    assert set(got) == set(want) | {"num_detected"}
    for k, v in want.items():
        if isinstance(v, np.ndarray):
            assert np.array_equal(got[k], v, equal_nan=True), k
        else:
            assert got[k] == v or (isinstance(v, float) and np.isnan(v) and np.isnan(got[k])), k
    print("rms", got["rms_reproj_error"], "fx", got["camera_matrix"][0, 0], "truth fx", cb.camera()[0][0, 0])
