"""GPU: the bird's-eye-view kernels (csrc/bev.hip: skimi_homography_fit, skimi_homography_points, skimi_warp_perspective_u8,
skimi_bev_skeleton, skimi_ground_track) and bev.py's chain against the float64 restatement (tests/bev_restated.py, itself held
against the reference's outputs and the exact four-point solve by tests/test_bev_cpu.py) on the cases of tests/bev_cases.py.
Every float64 output within 1e-9 (1 + |x|), the project's float64 tolerance; NaN masks, status, valid and px equal.  Warped
bytes equal the restatement except at near-tie bytes (unrounded value within 1e-6 of k + 0.5), which may differ by 1 and are
at most 1e-4 of a frame (asserted on the CPU)."""
import numpy as np
import pytest
import torch

import bev_cases as bc
import bev_restated as br
from skiing_analysis_pytorch_amd import bev, geometry, preprocess

pytestmark = pytest.mark.gpu
TOL = 1e-9


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def close(got, want, what):
    got = host(got) if isinstance(got, torch.Tensor) else got
    want = np.asarray(want, np.float64)
    assert got.shape == want.shape and got.dtype == np.float64, f"{what}: {got.shape} {got.dtype} against {want.shape}"
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN masks differ"
    with np.errstate(invalid="ignore"):
        e = np.abs(got - want) / (1 + np.abs(want))
    e[(got == want)] = 0.0                      # equal infinities
    err = np.nanmax(e) if np.isfinite(e).any() else 0.0
    print(f"{what}: max scaled error {err:.3g}")
    assert err <= TOL, what


def bits(*tensors):
    return b"".join(host(t).tobytes() for t in tensors)


def fit_bits(r):
    return bits(r.H, r.Hinv, r.Hn, r.err, r.stats, r.status)


def check_fit(src, dst, what, post=None):
    got = geometry.homography_fit(dev(src), dev(dst), post=post)
    want = br.homography_fit(src, dst, post)
    assert bool(host(got.status)) == want["status"], what
    for name in ("H", "Hinv", "Hn", "err", "stats"):
        close(getattr(got, name), want[name], f"{what} {name}")
    assert fit_bits(geometry.homography_fit(dev(src), dev(dst), post=post)) == fit_bits(got), f"{what}: a rerun differs"
    return got


# ---- the fit --------------------------------------------------------------------------------------------------------------
def test_fit_four_points():
    r = check_fit(bc.DEFAULT_IMG_PTS, bc.DEFAULT_BEV_PTS_M, "default points")
    assert bool(host(r.status)) and host(r.H)[2, 2] == 1.0 and host(r.err).max() < 1e-9
    check_fit(*bc.generic_quad(3), "generic quadrilateral")
    _, S = br.make_bev_canvas()
    p = check_fit(bc.DEFAULT_IMG_PTS, bc.DEFAULT_BEV_PTS_M, "default points, post = S", post=S)
    assert host(p.H)[2, 2] == 1.0
    assert np.abs(host(p.H) @ host(p.Hinv) - np.eye(3)).max() < 1e-12


@pytest.mark.parametrize("n", bc.FIT_NOISY_COUNTS)
def test_fit_least_squares(n):
    src, dst = bc.noisy_fit(n)
    r = check_fit(src, dst, f"n = {n}")
    assert bool(host(r.status)) and host(r.stats)[0] == n
    s2 = src.copy()
    s2[n // 2, 0] = np.nan                       # a NaN correspondence is skipped, and is NaN in err alone
    r2 = check_fit(s2, dst, f"n = {n}, one NaN")
    e = host(r2.err)
    assert np.isnan(e[n // 2]) and np.isfinite(np.delete(e, n // 2)).all() and host(r2.stats)[0] == n - 1


def test_fit_failures_stay_in_their_group():
    s3 = bc.DEFAULT_IMG_PTS.copy()
    s3[0, 0] = np.inf
    for src, dst, what in ((s3, bc.DEFAULT_BEV_PTS_M, "three usable points"), (*bc.collinear4(), "four collinear points"),
                           (np.ones((4, 2)), bc.DEFAULT_BEV_PTS_M, "coincident points")):
        r = check_fit(src, dst, what)
        assert not bool(host(r.status)) and np.isnan(host(r.H)).all() and np.isnan(host(r.Hinv)).all() and np.isnan(host(r.err)).all()
    # G = 3 with the failing group in the middle: the neighbours are bitwise what they are alone
    a, b = bc.generic_quad(1), bc.generic_quad(2)
    src, dst = np.stack([a[0], s3, b[0]]), np.stack([a[1], bc.DEFAULT_BEV_PTS_M, b[1]])
    batch = geometry.homography_fit(dev(src), dev(dst))
    assert host(batch.status).tolist() == [True, False, True] and np.isnan(host(batch.H[1])).all()
    for g, (s, d) in ((0, a), (2, b)):
        alone = geometry.homography_fit(dev(s), dev(d))
        assert bits(batch.H[g], batch.Hinv[g], batch.err[g], batch.stats[g]) == bits(alone.H, alone.Hinv, alone.err, alone.stats)
    # the same inside a batch of larger groups
    big = [bc.noisy_fit(65, seed=k) for k in range(3)]
    batch = geometry.homography_fit(dev(np.stack([s for s, _ in big])), dev(np.stack([d for _, d in big])))
    alone = geometry.homography_fit(dev(big[1][0]), dev(big[1][1]))
    assert bits(batch.H[1], batch.Hinv[1], batch.err[1], batch.stats[1]) == bits(alone.H, alone.Hinv, alone.err, alone.stats)


# ---- points ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", bc.POINT_COUNTS)
def test_points_match_restatement(n):
    x, H = bc.points_case(n)
    close(geometry.homography_points(dev(x), dev(H)), np.stack([br.homography_points(x[g], H[g]) for g in range(len(H))]),
          f"per-group H, n = {n}")
    close(geometry.homography_points(dev(x), dev(H[1])), br.homography_points(x, H[1]), f"shared H, n = {n}")
    close(bev.image_points_to_bev(dev(x[0]), dev(H[0]), eps=1e-3), br.homography_points(x[0], H[0], 1e-3), f"eps, n = {n}")


def test_points_bad_rows_stay_in_their_row():
    x, H = bc.points_case(65)
    ref = host(geometry.homography_points(dev(x), dev(H)))
    bad = x.copy()
    h = H[1]
    bad[1, 7] = [100.0, -(h[2, 0] * 100.0 + h[2, 2]) / h[2, 1]]      # on the line w = 0 of its group's matrix
    bad[0, 3, 1] = np.nan
    bad[2, 64, 0] = np.inf
    got = geometry.homography_points(dev(bad), dev(H))
    close(got, np.stack([br.homography_points(bad[g], H[g]) for g in range(3)]), "bad rows")
    got = host(got)
    rows = [(1, 7), (0, 3), (2, 64)]
    for g, j in rows:
        assert np.isnan(got[g, j]).all()
        ref[g, j] = got[g, j]
    assert got.tobytes() == ref.tobytes()


# ---- the warp -------------------------------------------------------------------------------------------------------------
def check_bytes(got, values, what):
    want = np.floor(values + 0.5).astype(np.uint8)
    diff = got.astype(np.int16) - want
    tie = br.near_tie(values)
    print(f"{what}: {int((diff != 0).sum())} bytes differ, {int(tie.sum())} near-tie bytes of {want.size}")
    assert (np.abs(diff) <= 1).all() and not (diff != 0)[~tie].any(), what


@pytest.mark.parametrize("name", list(bc.WARP_CASES))
def test_warp_matches_restatement(name):
    frames, Hinv, size, per_frame = bc.warp_case(name)
    C, F = frames.shape[:2]
    fd, guard = dev(frames), 4096
    buf = torch.full((C * F * size[0] * size[1] * frames.shape[-1] + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    out = buf[:-guard].view(C, F, size[1], size[0], frames.shape[-1])
    got = preprocess.warp_perspective(fd, dev(Hinv), size, per_frame=per_frame, out=out)
    assert got.data_ptr() == out.data_ptr()
    g = host(got)
    for c in range(C):
        for f in range(F):
            check_bytes(g[c, f], br.warp_values(frames[c, f], bc.frame_matrix(Hinv, per_frame, c, f), size), f"{name}[{c},{f}]")
    assert (host(buf[-guard:]) == 0xA5).all(), "the guard region behind the output was written"
    assert np.array_equal(host(fd), frames), "the input was modified"
    assert host(preprocess.warp_perspective(fd, dev(Hinv), size, per_frame=per_frame)).tobytes() == g.tobytes()
    if C == 1 and not per_frame:      # the four-axis form is the same launch
        assert host(preprocess.warp_perspective(fd[0], dev(Hinv[0]), size)).tobytes() == g[0].tobytes()


def test_warp_identity_translation_and_nan():
    rng = np.random.default_rng(9)
    for ch, (H, W) in ((3, (61, 97)), (1, (33, 70)), (4, (40, 52))):
        img = rng.integers(0, 256, (2, H, W, ch), dtype=np.uint8)
        d, eye = dev(img), torch.eye(3, dtype=torch.float64, device="cuda")
        assert np.array_equal(host(preprocess.warp_perspective(d, eye, (W, H))), img)
        crop = host(preprocess.warp_perspective(d, eye * -2.5, (W - 5, H - 7)))
        assert np.array_equal(crop, img[:, :H - 7, :W - 5])
        pad = host(preprocess.warp_perspective(d, eye, (W + 9, H + 3)))
        assert np.array_equal(pad[:, :H, :W], img) and not pad[:, H:].any() and not pad[:, :, W:].any()
        shift = dev(np.array([[1.0, 0, 3], [0, 1, -2], [0, 0, 1]]))
        moved = host(preprocess.warp_perspective(d, shift, (W, H)))
        assert np.array_equal(moved[:, 2:, :W - 3], img[:, :H - 2, 3:]) and not moved[:, :2].any() and not moved[:, :, W - 3:].any()
        # a NaN matrix (a failed fit) gives a zero frame and leaves the other frame's bits alone
        mats = torch.stack([shift, torch.full((3, 3), float("nan"), dtype=torch.float64, device="cuda")])
        both = host(preprocess.warp_perspective(d, mats, (W, H), per_frame=True))
        assert np.array_equal(both[0], moved[0]) and not both[1].any()


# ---- the skeleton and the track ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("J", (17, 21))
@pytest.mark.parametrize("T", (1, 2, 243))
def test_skeleton_matches_restatement(T, J):
    X, cpx = bc.skeleton_case(T, J)
    for rot, axes, mpp in ((True, (0, 2), 0.02), (False, (0, 1), 0.05)):
        got = geometry.bev_skeleton(dev(X), dev(cpx), mpp, axes, rot)
        uv, px, valid, cw = br.bev_skeleton(X, cpx, mpp, axes, rot)
        close(got.uv, uv, f"uv T={T} J={J}")
        close(got.center_world, cw, f"center_world T={T} J={J}")
        assert np.array_equal(host(got.valid), valid) and np.array_equal(host(got.px), px)
        assert host(got.px).dtype == np.int32 and not host(got.px)[~valid].any()
    if T > 2:
        assert not host(got.valid)[T // 2].any() and np.isnan(host(got.center_world)[T // 2]).all()


def test_skeleton_half_way_values_and_given_centre():
    X, cpx, mpp = bc.halfway_case()
    got = geometry.bev_skeleton(dev(X), dev(cpx), mpp, (0, 2), True)
    uv, px, valid, cw = br.bev_skeleton(X, cpx, mpp, (0, 2), True)
    assert np.array_equal(host(got.uv), uv, equal_nan=True) and np.array_equal(host(got.px), px) and np.array_equal(host(got.valid), valid)
    frac = uv[valid] - np.floor(uv[valid])
    assert (frac == 0.5).sum() >= 10
    # project_world_to_bev_centered with the caller's centre, one step
    c = np.array([0.125, -0.25, 0.375])
    one = bev.project_world_to_bev_centered(dev(X[0]), dev(c), (400, 800), mpp, rot90_left=False)
    uv1, px1, valid1 = br.project_world_to_bev_centered(X[0], c, (400, 800), mpp, (0, 2), False)
    assert np.array_equal(host(one.px), px1) and np.array_equal(host(one.valid), valid1) and np.array_equal(host(one.uv), uv1)


@pytest.mark.parametrize("T", (1, 2, 243))
def test_ground_track_matches_restatement(T):
    p = bc.track_case(2, T)
    got = geometry.ground_track(dev(p), 30.0)
    want = br.ground_track(p, 30.0)
    close(got.table, want, f"track T={T}")
    assert bits(geometry.ground_track(dev(p), 30.0).table) == bits(got.table)
    alone = geometry.ground_track(dev(p[1]), 30.0)
    assert bits(alone.table) == bits(got.table[1]) and tuple(alone.velocity.shape) == (T, 2)


# ---- end to end -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def clip():
    frames, boxes, X = bc.front_clip_case()
    return frames, boxes, X, br.process_front_clip(frames, boxes, skeleton=X)


def test_process_front_clip_matches_restated_chain(clip):
    frames, boxes, X, want = clip
    got = bev.process_front_clip(dev(frames), dev(boxes), skeleton=dev(X))
    assert bool(host(got.status)) and got.bev_size == (800, 1600) and tuple(got.bev.shape) == (3, 1600, 800, 3)
    for name in ("foot_uv", "foot_px", "foot_m", "H_px", "H_m"):
        close(getattr(got, name), want[name], name)
    close(got.track.table, want["track"], "track")
    uv, px, valid, cw = want["skeleton"]
    close(got.skeleton.uv, uv, "skeleton uv")
    assert np.array_equal(host(got.skeleton.px), px) and np.array_equal(host(got.skeleton.valid), valid)
    g = host(got.bev)
    for t in range(3):
        check_bytes(g[t], want["values"][t], f"bev frame {t}")
    blank = bev.process_front_clip(dev(frames), dev(boxes), blank_bev=True)
    assert (host(blank.bev) == 10).all() and bits(blank.foot_px) == bits(got.foot_px)
    # smooth= acts on the metric track alone: the track is that of the smoothed foot points, everything else as before
    X3 = torch.cat([got.foot_m, torch.zeros_like(got.foot_m[..., :1])], dim=-1)
    for how, smoothed in (("ema", geometry.smooth_ema(X3).X), ("savgol", geometry.smooth_savgol(X3).X)):
        s = bev.process_front_clip(dev(frames), dev(boxes), blank_bev=True, smooth=how)
        close(s.track.table, br.ground_track(np.transpose(host(smoothed)[..., :2], (1, 0, 2)), 30.0), f"track, smooth = {how}")
        assert bits(s.foot_m) == bits(got.foot_m) and bits(s.foot_px) == bits(got.foot_px)


def test_make_bev_matches_restated_chain():
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (1080, 1920, 3), dtype=np.uint8)
    boxes = np.array([[400.0, 300.0, 520.0, 700.0], [900.0, 500.0, 1000.0, 900.0]])
    d_img = dev(img)
    foot, src, bev_img = bev.make_bev(d_img, dev(boxes))
    size, S = br.make_bev_canvas()
    fit = br.homography_fit(br.DEFAULT_IMG_PTS, br.DEFAULT_BEV_PTS_M, S)
    close(foot, br.homography_points(br.foot_from_bbox_xyxy(boxes), fit["H"]), "make_bev foot_xy_px")
    assert src is d_img and np.array_equal(host(src), img)
    values = br.warp_values(img, fit["Hinv"], size)
    assert br.near_tie(values).sum() <= 1e-4 * values.size
    check_bytes(host(bev_img), values, "make_bev bev_img")
    _, _, blank = bev.make_bev(dev(img), dev(boxes[0]), blank_bev=True)
    assert tuple(blank.shape) == (1600, 800, 3) and (host(blank) == 10).all()
    with pytest.raises(ValueError):
        bev.make_bev(dev(img), dev(boxes), img_pts=bc.collinear4()[0])
