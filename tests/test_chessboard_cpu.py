"""No GPU: the chessboard detector's rules (tests/chessboard_restated.py) against the truth of rendered boards
(tests/chessboard_cases.py), calibration.order_chessboard on synthetic grids, the two wrappers' refusal of host tensors, and
calibrate_from_frames' failure dictionary with the detection stubbed out."""
from pathlib import Path

import numpy as np
import pytest
import torch

import chessboard_cases as cb
import chessboard_restated as cs
from skiing_analysis_pytorch_amd import _lib, calibration, geometry


# ---- the restatement against the rendered truth -------------------------------------------------------------------------
def test_ring_offsets_follow_the_formula():
    assert cs.ring_offsets() == cs.RING


@pytest.mark.parametrize("view", cb.VIEWS)
def test_restatement_finds_every_corner_of_a_rendered_board(view):
    board, cand, pts, ok = cb.restated(view)
    assert int(cand["count"]) >= 54 and board is not None, (view, int(cand["count"]))
    err = np.hypot(*(board - cb.canonical(cb.truth(view))).T)
    print(f"view {view}: candidates {int(cand['count'])}, mean {err.mean():.3f} px, worst {err.max():.3f} px")
    assert err.max() <= cb.TRUTH_BOUND_PX, (view, err.max())


def test_a_board_half_outside_the_frame_is_not_found():
    board, cand, _, _ = cb.restated(0, cb.HALF_OUT_SHIFT)
    assert board is None and 0 < int(cand["count"]) < 54


def test_candidate_rules_on_small_frames():
    flat = cs.candidates(np.full((40, 50, 3), 90, np.uint8))
    assert int(flat["count"]) == 0 and int(flat["rmax"]) == 0 and (flat["xy"] == -1).all() and (flat["response"] == 0).all()
    noise = cs.candidates(cb.noise_frame(), max_candidates=64)
    n = int(noise["count"])
    assert n > 64 and (noise["xy"] >= 0).all()
    lin = noise["xy"][:, 1].astype(np.int64) * cb.noise_frame().shape[1] + noise["xy"][:, 0]
    assert (np.diff(lin) > 0).all()                                   # ascending pixel order
    full = cs.candidates(cb.noise_frame(), max_candidates=n + 3)
    assert np.array_equal(full["xy"][:64], noise["xy"]) and (full["xy"][n:] == -1).all()
    tiny = cs.candidates(np.zeros((12, 30), np.uint8))                # no pixel is 6 px from every edge
    assert int(tiny["count"]) == 0


def test_ties_go_to_the_earlier_pixel():
    """a frame that is its own mirror image has pairs of equal responses: within one window only the earlier pixel stays"""
    g = cb.render(0)[100:160, 200:260]
    sym = np.concatenate([g, g[:, ::-1]], axis=1)
    c = cs.candidates(sym, nms_radius=4)
    R = cs.response(sym)
    xy = c["xy"][:int(c["count"])]
    for x, y in xy:
        win = R[max(y - 4, 0):y + 5, max(x - 4, 0):x + 5]
        assert R[y, x] == win.max()
        ys, xs = np.nonzero(win == R[y, x])
        first = (ys[0] + max(y - 4, 0), xs[0] + max(x - 4, 0))
        assert first == (y, x)


def test_subpix_special_points():
    img = cb.render(0)
    pts, ok = cs.corner_subpix(img, [cb.FLAT_POINT, [np.nan, 3.0], [-1.0, 4.0], [640.0, 10.0], cb.far_point(0)])
    assert ok.tolist() == [True, False, False, False, False]          # a flat patch (singular system) stays and is no revert
    assert np.array_equal(pts[0], cb.FLAT_POINT) and np.isnan(pts[1, 0]) and np.array_equal(pts[4], cb.far_point(0))
    board, cand, pts, good = cb.restated(0)
    k = int(cand["count"])
    moved = np.hypot(*(pts[:k] - cand["xy"][:k]).T)
    assert good.all() and (moved < 1.5).all() and (moved > 0).any()
    # a corner 2 px from the frame's edge: the window reaches over the replicated border, which costs one arm of the corner
    # (so the truth's bound is not asked of it); the point still converges within a pixel and differs from the uncropped one
    frame, start, want = cb.border_case()
    got, ok = cs.corner_subpix(frame, [start], win=cb.WIN)
    x0 = cb.render(0).shape[1] - frame.shape[1]
    whole, _ = cs.corner_subpix(img, [start + [x0, 0.0]], win=cb.WIN)
    assert ok[0] and np.hypot(*(got[0] - want)) < 1.0 and np.hypot(*(whole[0] - [x0, 0.0] - want)) <= cb.TRUTH_BOUND_PX
    assert not np.array_equal(got[0], whole[0] - [x0, 0.0])
    # only the first `count` points are refined
    pts, ok = cs.corner_subpix(img, cand["xy"][:4], count=2)
    assert ok.tolist() == [True, True, False, False] and np.array_equal(pts[2:], cand["xy"][2:4])


# ---- order_chessboard ----------------------------------------------------------------------------------------------------
def grid(cols=9, rows=6, ring=0):
    """a board under a mild homography, row-major with `cols` corners a row, first corner top-left, right-handed; ring = 1:
    with the ring of cells that would continue it"""
    u, v = np.meshgrid(np.arange(-ring, cols + ring, dtype=np.float64), np.arange(-ring, rows + ring, dtype=np.float64))
    w = 1.0 + 0.02 * u + 0.015 * v
    x, y = 100 + (30 * u + 4 * v) / w, 80 + (-3 * u + 28 * v) / w
    return np.stack([x, y], -1).reshape(-1, 2)


def test_order_recovers_a_shuffled_board_among_distractors():
    g = grid()
    rng = np.random.default_rng(3)
    for trial in range(4):
        extra = rng.uniform([20, 20], [420, 300], (40, 2))
        # not on the board and not where the grid would go on: a point there continues the grid, and the rule refuses that
        extra = extra[np.hypot(*(extra[:, None] - grid(ring=1)[None]).transpose(2, 0, 1)).min(axis=1) > 12][:6]
        assert len(extra) == 6
        pts = np.concatenate([g, extra])
        perm = rng.permutation(len(pts))
        got = calibration.order_chessboard(pts[perm], (9, 6), strength=rng.uniform(1, 2, len(pts)))
        assert got is not None and np.array_equal(got, g), trial


def test_order_needs_every_corner_and_no_more():
    g = grid()
    assert calibration.order_chessboard(np.delete(g, 20, axis=0), (9, 6)) is None
    assert calibration.order_chessboard(np.delete(g, 0, axis=0), (9, 6)) is None
    assert calibration.order_chessboard(g, (8, 6)) is None and calibration.order_chessboard(g, (9, 7)) is None
    assert calibration.order_chessboard(g[:4], (9, 6)) is None and calibration.order_chessboard(np.zeros((0, 2)), (9, 6)) is None
    with pytest.raises(ValueError, match="at least 2 x 2"):
        calibration.order_chessboard(g, (9, 1))


def test_order_drops_the_weaker_of_two_points_within_a_pixel_and_skips_non_finite_rows():
    g = grid()
    pts = np.concatenate([g, g[[7]] + [0.6, 0.0], [[np.nan, 5.0]]])
    s = np.concatenate([np.full(len(g), 2.0), [1.0, 3.0]])
    assert np.array_equal(calibration.order_chessboard(pts, (9, 6), strength=s), g)
    s[7], s[len(g)] = 1.0, 2.0                                        # now the shifted twin is the stronger one
    got = calibration.order_chessboard(pts, (9, 6), strength=s)
    want = g.copy()
    want[7] += [0.6, 0.0]
    assert np.array_equal(got, want)


def test_order_normalisation():
    g = grid()
    # the same points described as a 6 x 9 board: the columns run along the short side, right-handed, first corner by (y, x)
    t = calibration.order_chessboard(g, (6, 9)).reshape(9, 6, 2)
    col, row = t[0, 1] - t[0, 0], t[1, 0] - t[0, 0]
    assert col[0] * row[1] - col[1] * row[0] > 0
    assert sorted(map(tuple, t.reshape(-1, 2))) == sorted(map(tuple, g))
    other = t[::-1, ::-1][0, 0]
    assert (t[0, 0, 1], t[0, 0, 0]) < (other[1], other[0])
    # the 180-degree rule: the board turned upside down in the image comes back as the same list
    c = g.mean(axis=0)
    turned = 2 * c - g
    got = calibration.order_chessboard(turned, (9, 6))
    want = turned[::-1]                                               # = the turned board read from its new top-left
    assert np.array_equal(got, want) and (got[0, 1], got[0, 0]) < (got[-1, 1], got[-1, 0])
    # a mirrored board (seen from behind) is still returned right-handed
    mirrored = g * [-1.0, 1.0] + [600.0, 0.0]
    m = calibration.order_chessboard(mirrored, (9, 6)).reshape(6, 9, 2)
    col, row = m[0, 1] - m[0, 0], m[1, 0] - m[0, 0]
    assert col[0] * row[1] - col[1] * row[0] > 0


# ---- the wrappers refuse host tensors before the library is touched ------------------------------------------------------
def test_new_names_are_public():
    for name in ("chessboard_candidates", "corner_subpix", "ChessCandidates", "SubpixResult", "CHESS_MAX_NMS", "SUBPIX_MAX_WIN",
                 "SUBPIX_MAX_ITERS"):
        assert hasattr(geometry, name), name
    for name in ("order_chessboard", "find_chessboard_corners", "calibrate_from_frames"):
        assert callable(getattr(calibration, name)), name


HOST_CALLS = {
    "chessboard_candidates": lambda: geometry.chessboard_candidates(torch.zeros(2, 16, 16, 3, dtype=torch.uint8)),
    "corner_subpix": lambda: geometry.corner_subpix(torch.zeros(2, 16, 16, 3, dtype=torch.uint8), torch.zeros(2, 4, 2)),
}


@pytest.mark.parametrize("name", sorted(HOST_CALLS))
def test_wrapper_refuses_host_tensors(name, monkeypatch):
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", Path("no_such_dir") / "libskimi.so")
    with pytest.raises(_lib.SkimiError, match=name):
        HOST_CALLS[name]()


# ---- calibrate_from_frames -----------------------------------------------------------------------------------------------
def test_calibrate_from_frames_reports_no_corners(monkeypatch):
    seen = {}

    def no_board(frames, board_size, win=(11, 11)):
        seen["args"] = (tuple(frames.shape), board_size, win)
        return np.full((3, 54, 2), np.nan), np.zeros(3, bool)

    monkeypatch.setattr(calibration, "find_chessboard_corners", no_board)
    got = calibration.calibrate_from_frames(torch.zeros(3, 36, 64, 3, dtype=torch.uint8), calibration.CalibConfig())
    assert got == {"status": "Failed", "reason": "No corners detected", "num_images": 0}
    assert seen["args"] == ((3, 36, 64, 3), (9, 6), (11, 11))
    with pytest.raises(ValueError, match="2 names for 3 frames"):
        calibration.calibrate_from_frames(torch.zeros(3, 36, 64, 3, dtype=torch.uint8), calibration.CalibConfig(), names=["a", "b"])


def test_calibrate_from_frames_hands_the_detected_boards_on(monkeypatch):
    corners = np.arange(4 * 54 * 2, dtype=np.float64).reshape(4, 54, 2)
    corners[2] = np.nan
    seen = {}

    def solver(c, cfg, image_size=None, names=None, undistort=None):
        seen.update(corners=c, size=image_size, names=names)
        return {"status": "Success", "used_names": list(names)}

    monkeypatch.setattr(calibration, "find_chessboard_corners", lambda *a, **k: (corners, np.array([True, True, False, True])))
    monkeypatch.setattr(calibration, "calibrate_camera", solver)
    got = calibration.calibrate_from_frames(torch.zeros(4, 36, 64, 1, dtype=torch.uint8), calibration.CalibConfig(), names=list("abcd"))
    assert got == {"status": "Success", "used_names": ["a", "b", "d"], "num_detected": 3}
    assert seen["size"] == (64, 36) and seen["names"] == ["a", "b", "d"] and np.array_equal(seen["corners"], corners[[0, 1, 3]])
