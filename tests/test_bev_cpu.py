"""CPU: the restatement of the bird's-eye view (tests/bev_restated.py) against the reference's own outputs (tests/golden/
bev.npz, written by tools/make_goldens.py bev from front_side/front/bev_utils.py, front/run.py and front_side/run.py), the
restated fit against the exact four-point solve, and the near-tie condition that lets the GPU test compare warped bytes
for equality.  cv2.findHomography and cv2.warpPerspective are not pinned against cv2 (it is not installed where the
goldens are made): the fit is pinned by the exact solve here, the warp by its rule (include/skimi.h).

The three bounds of the fit are 10 x the worst value measured over the 51 cases below (profiles/bev.md):
  restated H against np.linalg.solve's, |dH| / (1 + |H|)      worst 3.05e-14
  transfer error of the four points, in metres                 worst 7.82e-14
  max |H Hinv - I|                                             worst 1.79e-14
"""
from pathlib import Path

import numpy as np
import pytest
import torch

import bev_cases as bc
import bev_restated as br
from skiing_analysis_pytorch_amd import _lib, bev, geometry, preprocess

GOLD = Path(__file__).parent / "golden" / "bev.npz"
FIT_BOUND, MAP_BOUND, INV_BOUND = 3.1e-13, 7.9e-13, 1.8e-13
TIE_SHARE = 1e-4


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLD, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def test_pure_functions_reproduce_the_reference(gold):
    for cfg, size, S in zip(gold["canvas_cfg"], gold["canvas_size"], gold["canvas_S"]):
        got_size, got_S = br.make_bev_canvas(*map(float, cfg))
        assert tuple(got_size) == tuple(size) and np.abs(got_S - S).max() <= 1e-12
        prod_size, prod_S = bev.make_bev_canvas(bev.BeVConfig(*map(float, cfg)))      # the product's host function too
        assert tuple(prod_size) == tuple(size) and np.array_equal(prod_S, got_S)
    assert np.abs(br.foot_from_bbox_xyxy(gold["foot_boxes"]) - gold["foot_out"]).max() <= 1e-12
    got = br.homography_points(gold["pts_uv"], gold["pts_H"])
    assert np.abs(got - gold["pts_out"]).max() <= 1e-12
    xyxy = br.convert_xywh_to_xyxy(gold["xywh"])
    assert np.abs(xyxy - gold["xyxy"]).max() <= 1e-12
    assert np.abs(br.unnormalize_bbox(xyxy, tuple(gold["unnorm_size"])) - gold["unnorm_out"]).max() <= 1e-12
    assert np.array_equal(bev.DEFAULT_IMG_PTS, br.DEFAULT_IMG_PTS) and np.array_equal(bev.DEFAULT_BEV_PTS_M, br.DEFAULT_BEV_PTS_M)


def test_skeleton_on_the_plan_reproduces_the_reference(gold):
    halves = 0
    for k in range(int(gold["skel_count"])):
        g = {key: gold[f"skel{k}_{key}"] for key in ("X", "center_world", "center_px", "mpp", "axes", "rot", "px", "valid")}
        uv, px, valid = br.project_world_to_bev_centered(g["X"], g["center_world"], g["center_px"], float(g["mpp"]),
                                                         tuple(g["axes"]), bool(g["rot"]))
        assert np.array_equal(valid, g["valid"]) and np.array_equal(px, g["px"]), k
        assert not valid[3] and not valid[7] and np.isnan(uv[3]).all()
        frac = uv[valid] - np.floor(uv[valid])
        halves += int((frac == 0.5).sum())
    assert halves >= 10, "the fixture is meant to exercise round-half-to-even"


def _fit_cases():
    return [(bc.DEFAULT_IMG_PTS, bc.DEFAULT_BEV_PTS_M)] + [bc.generic_quad(s) for s in range(bc.N_QUADS)]


def test_restated_fit_is_the_exact_four_point_homography():
    worst = np.zeros(3)
    for src, dst in _fit_cases():
        f = br.homography_fit(src, dst)
        assert f["status"] and f["stats"][0] == 4
        exact = br.homography_exact4(src, dst)
        worst = np.maximum(worst, [(np.abs(f["H"] - exact) / (1 + np.abs(exact))).max(), f["err"].max(),
                                   np.abs(f["H"] @ f["Hinv"] - np.eye(3)).max()])
        assert f["H"][2, 2] == 1.0
    print("worst |dH| / (1 + |H|) %.3g, transfer error %.3g m, |H Hinv - I| %.3g" % tuple(worst))
    assert worst[0] <= FIT_BOUND and worst[1] <= MAP_BOUND and worst[2] <= INV_BOUND


def test_restated_fit_rules():
    src, dst = bc.noisy_fit(64)
    f = br.homography_fit(src, dst)
    assert f["status"] and 0.0 < f["stats"][1] < 1.0          # 0.5 px of image noise is centimetres on the ground
    # a NaN correspondence is skipped: the same as the fit without it
    s2, d2 = src.copy(), dst.copy()
    s2[5, 1] = np.nan
    g = br.homography_fit(s2, d2)
    h = br.homography_fit(np.delete(src, 5, 0), np.delete(dst, 5, 0))
    assert g["stats"][0] == 63 and np.isnan(g["err"][5]) and np.array_equal(g["H"], h["H"])
    # three usable points, coincident points and collinear points fail
    s3 = bc.DEFAULT_IMG_PTS.copy()
    s3[0, 0] = np.inf
    for bad in (br.homography_fit(s3, bc.DEFAULT_BEV_PTS_M), br.homography_fit(np.ones((4, 2)), bc.DEFAULT_BEV_PTS_M),
                br.homography_fit(*bc.collinear4())):
        assert not bad["status"] and np.isnan(bad["H"]).all() and np.isnan(bad["Hinv"]).all() and np.isnan(bad["err"]).all()
    # post composes on the left and the error is measured in post's frame
    _, S = br.make_bev_canvas()
    fm, fp = br.homography_fit(bc.DEFAULT_IMG_PTS, bc.DEFAULT_BEV_PTS_M), br.homography_fit(bc.DEFAULT_IMG_PTS, bc.DEFAULT_BEV_PTS_M, S)
    assert np.array_equal(fp["H"], br.compose3(S, fm["H"])) and fp["H"][2, 2] == 1.0 and fp["stats"][3] == fm["stats"][3]
    corners = br.homography_points(bc.DEFAULT_IMG_PTS, fp["H"])
    assert np.abs(corners - [[100, 1400], [700, 1400], [700, 200], [100, 200]]).max() < 1e-9


def _warp_frames():
    for name in bc.WARP_CASES:
        frames, Hinv, size, per_frame = bc.warp_case(name)
        for c in range(frames.shape[0]):
            for f in range(frames.shape[1]):
                yield f"{name}[{c},{f}]", frames[c, f], bc.frame_matrix(Hinv, per_frame, c, f), size
    frames, boxes, _ = bc.front_clip_case()
    chain = br.process_front_clip(frames, boxes)
    for t in range(len(frames)):
        yield f"front_clip[{t}]", None, chain["values"][t], None


def test_near_tie_condition_on_every_warp_case():
    """what entitles test_bev_gpu.py to compare bytes: at most 1e-4 of a frame's bytes have an unrounded value within
    1e-6 of k + 0.5"""
    for what, frame, G, size in _warp_frames():
        values = G if frame is None else br.warp_values(frame, G, size)
        ties = int(br.near_tie(values).sum())
        print(f"{what}: {ties} near-tie bytes of {values.size}, {float((values > 0).mean()):.2f} of the frame covered")
        assert ties <= TIE_SHARE * values.size, what
        assert 0.2 < (values > 0).mean() < 0.95, f"{what}: the case is meant to cover the frame AND leave it"


def test_restated_warp_rules():
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (23, 31, 3), dtype=np.uint8)
    same = br.warp_perspective(img, np.eye(3), (31, 23))
    assert np.array_equal(same, img)
    padded = br.warp_perspective(img, np.eye(3) * -2.5, (40, 20))          # a homography's scale and sign are free
    assert np.array_equal(padded[:, :31], img[:20]) and not padded[:, 31:].any()
    shift = np.array([[1.0, 0, 3], [0, 1, -2], [0, 0, 1]])
    moved = br.warp_perspective(img, shift, (31, 23))
    assert np.array_equal(moved[2:, :28], img[:21, 3:]) and not moved[:2].any() and not moved[:, 28:].any()
    assert not br.warp_perspective(img, np.full((3, 3), np.nan), (31, 23)).any()


def test_restated_track_and_skeleton_rules():
    p = bc.track_case(2, 243)
    tr = br.ground_track(p, 30.0)
    assert np.array_equal(tr[:, 0, 0], [0.0, 0.0]) and np.isnan(tr[0, 5, 0]) and np.isnan(tr[0, 6, 0]) and np.isnan(tr[0, 4, 2])
    fin = np.isfinite(tr[..., 0])
    assert np.allclose(tr[..., 1][:, -1], np.where(fin, tr[..., 0], 0.0).sum(1)) and (np.diff(tr[..., 1], axis=1) >= 0).all()
    assert np.isnan(br.ground_track(bc.track_case(2, 1), 30.0)[..., 2:]).all()
    # a straight run down the lane at 9 m/s: heading atan2(0, -9) = pi
    line = np.stack([np.zeros(10), 50.0 - 0.3 * np.arange(10)], -1)[None]
    tr = br.ground_track(line, 30.0)
    assert np.allclose(tr[0, :, 4], 9.0) and np.allclose(tr[0, :, 5], np.pi) and np.allclose(tr[0, -1, 1], 2.7)
    X, cpx, mpp = bc.halfway_case()
    uv, px, valid, cw = br.bev_skeleton(X, cpx, mpp, (0, 2), True)
    assert np.array_equal(cw[0], np.zeros(3)) and valid[0].all() and not valid[1, 2]
    frac = uv[valid] - np.floor(uv[valid])
    assert (frac == 0.5).sum() >= 10 and np.array_equal(px[valid], np.rint(uv[valid]).astype(np.int32))
    assert (px[valid][frac[:, 0] == 0.5][:, 0] % 2 == 0).all()


def test_cpu_tensors_are_rejected():
    x = torch.zeros(4, 2, dtype=torch.float64)
    for call in (lambda: geometry.homography_fit(x, x), lambda: geometry.homography_points(x, torch.eye(3, dtype=torch.float64)),
                 lambda: geometry.bev_skeleton(torch.zeros(2, 17, 3), torch.zeros(2, 2)), lambda: geometry.ground_track(x),
                 lambda: preprocess.warp_perspective(torch.zeros(1, 4, 4, 3, dtype=torch.uint8), torch.eye(3), (4, 4)),
                 lambda: bev.process_front_clip(torch.zeros(1, 4, 4, 3, dtype=torch.uint8), torch.zeros(1, 1, 4)),
                 lambda: bev.make_bev(torch.zeros(4, 4, 3, dtype=torch.uint8), torch.zeros(1, 4)),
                 lambda: bev.foot_from_bbox_xyxy(torch.zeros(4))):
        with pytest.raises(_lib.SkimiError):
            call()
