"""GPU: the SIFT-style features and the L2 matcher (csrc/sift.hip: sift_blur_kernel, sift_half_kernel, sift_count_kernel,
sift_write_kernel, sift_refine_kernel, sift_select_kernel, sift_describe_kernel, l2_nn_kernel, l2_keep_kernel;
geometry.sift_features, geometry.match_l2, camera_position.estimate_camera_pose(s)_from_SIFT, estimate_pose_from_bbox_region)
against the restatement tests/sift_restated.py on the frames of tests/sift_cases.py.

Bounds.  The scale space is float32 in one stated operation order and the refinement float64 with + - * / only, so count,
octave_count, octave, layer, xy_level, xy, sigma, response and everything of match_l2 are bitwise equal.  The orientation and
the descriptor go through exp, atan2, cos and sin: angle within 1e-9; a descriptor byte equals the rounded restated value where
that value is farther than 1e-6 from a half-integer and differs by at most 1 elsewhere (tests/test_sift_cpu.py asserts that the
restatement has no orientation margin under 1e-9 and at most 1e-4 of the entries that close to a half-integer on these
frames).  The pose: R, T within 1e-9 (1 + |x|) of tests/essential_restated.py fed with the restated matches; against the truth
within sift_cases.ROT_BOUND_DEG, DIR_BOUND_DEG."""
import numpy as np
import pytest
import torch

import features_cases as fc
import sift_cases as sc
import sift_restated as sr
from skiing_analysis_pytorch_amd import _lib, camera_position, geometry

dev = lambda a: torch.from_numpy(np.array(a)).cuda()   # noqa: E731  (a copy: the cached frames are read-only)
EXACT = ("count", "octave_count", "octave", "layer", "xy_level", "xy", "sigma", "response")
NAMES = sorted(sc.frames())
TWO_PI = 2 * np.pi


def got_features(frames, *a, **kw):
    r = geometry.sift_features(dev(frames), *a, **kw)
    assert r.xy.dtype == torch.float64 and r.desc.dtype == torch.uint8 and r.count.dtype == torch.int32
    return {k: getattr(r, k).cpu().numpy() for k in r._fields}


def same_features(got, want, what):
    for k in EXACT:
        assert np.array_equal(got[k], want[k]), (what, k, got["count"], want["count"], got["octave_count"], want["octave_count"])
    n = int(want["count"])
    d = np.abs(got["angle"][:n] - want["angle"][:n])
    assert (np.minimum(d, TWO_PI - d) <= 1e-9).all(), (what, "angle", float(np.minimum(d, TWO_PI - d).max()))
    assert (got["angle"][n:] == -1.0).all() and not got["desc"][n:].any()
    v = want["desc_value"][:n]
    far = np.abs(v - np.floor(v) - 0.5) > 1e-6
    diff = np.abs(got["desc"][:n].astype(np.int64) - want["desc"][:n].astype(np.int64))
    assert (diff[far] == 0).all() and (diff <= 1).all(), (what, "desc", int(diff.max()), int((diff[far] != 0).sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_features_are_the_restatement(name):
    M = sc.max_features_of(name)
    got = got_features(sc.frames()[name][None], M)
    want = sc.restated(name, M)
    O = len(want["octave_count"])
    assert got["xy"].shape == (1, M, 2) and got["desc"].shape == (1, M, 128) and got["octave_count"].shape == (1, O)
    same_features({k: v[0] for k, v in got.items()}, want, name)
    print(name, "count", got["count"][0], "octaves", got["octave_count"][0])
    if name in ("constant", "tiny_15x15", "small_40x36"):
        assert got["count"][0] == 0
    if name == "tiny_15x15":
        assert O == 0
    if name == "small_40x36":
        assert O == 2
    if name == "blobs":
        assert got["count"][0] == M < got["octave_count"][0].sum()


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [dict(max_features=1), dict(max_features=37), dict(max_features=4096), dict(max_features=37, octaves=1),
                                dict(max_features=300, octaves=3), dict(max_features=50, octaves=8)])
def test_other_quotas_and_octaves(kw):
    for name in ("crop_317x211", "tiled"):
        got = got_features(sc.frames()[name][None], **kw)
        want = sr.sift_features(sc.frames()[name], **kw)
        same_features({k: v[0] for k, v in got.items()}, want, (name, kw))
        assert want["count"] == min(kw["max_features"], want["count"]) and want["count"] >= min(kw["max_features"], 37)


@pytest.mark.gpu
def test_a_batch_is_bitwise_its_frames_alone_and_a_rerun():
    clip = np.stack([np.stack(fc.view_pair(p[0])) for p in fc.PAIRS])[..., None]          # [3, 2, H, W, 1]
    clip = np.ascontiguousarray(clip.transpose(1, 0, 2, 3, 4))                            # [C = 2, F = 3, H, W, 1]
    batch, again = got_features(clip, 120), got_features(clip, 120)
    assert batch["xy"].shape == (2, 3, 120, 2) and batch["count"].shape == (2, 3) and batch["octave_count"].shape == (2, 3, 4)
    assert (batch["count"] == 120).all()
    for k in batch:
        assert np.array_equal(batch[k], again[k]), ("rerun", k)
    for c in range(2):
        for f in range(3):
            alone = got_features(clip[c, f][None], 120)
            for k in batch:
                assert np.array_equal(batch[k][c, f], alone[k][0]), (c, f, k)
    flat = got_features(clip.reshape(6, fc.H, fc.W, 1), 120)
    for k in batch:
        assert np.array_equal(batch[k].reshape(flat[k].shape), flat[k]), ("four axes", k)


@pytest.mark.gpu
def test_roi_keeps_the_keypoints_of_a_box():
    name = "roll-20_in_a_ch3"
    frame = sc.frames()[name]
    boxes = np.array([[60.0, 40.5, 250.0, 200.0], [0.0, 0.0, fc.W, fc.H], [100.0, 50.0, np.nan, 200.0], [200.0, 100.0, 100.0, 200.0],
                      [-np.inf, -np.inf, np.inf, 120.0]])
    got = got_features(np.stack([frame] * len(boxes)), sc.MAX_FEATURES, roi=dev(boxes))
    for i, box in enumerate(boxes):
        want = sr.sift_features(frame, sc.MAX_FEATURES, roi=box)
        same_features({k: v[i] for k, v in got.items()}, want, (name, i))
        n = got["count"][i]
        xy = got["xy"][i, :n]
        assert ((xy[:, 0] >= box[0]) & (xy[:, 0] < box[2]) & (xy[:, 1] >= box[1]) & (xy[:, 1] < box[3])).all()
    assert got["count"][0] > 30 and got["count"][2] == 0 and got["count"][3] == 0 and got["count"][4] > 30
    same_features({k: v[1] for k, v in got.items()}, sc.restated(name), "the whole frame as a box")


def got_matches(d1, n1, d2, n2, **kw):
    r = geometry.match_l2(dev(d1), dev(np.asarray(n1, np.int32)), dev(d2), dev(np.asarray(n2, np.int32)), **kw)
    assert all(t.dtype == torch.int32 for t in r)
    return [t.cpu().numpy() for t in r]


@pytest.mark.gpu
@pytest.mark.parametrize("kw", sc.MATCH_MODES)
def test_matcher_is_bitwise_the_restatement(kw):
    """set sizes 0, 1, 2, 5, around the wave (63, 65), the query block and the train tile (64), the sort's wave span (257)
    and beyond (513, 600); duplicated rows (s1 = s2 = 0, index ties); one call for all pairs of sets, the rows behind n1, n2
    hold noise"""
    d1, d2 = sc.match_sets()
    sizes = sc.MATCH_SIZES
    full = dict(dict(ratio=None, cross_check=False, max_distance2=None), **kw)
    for mm in (9, 700):
        pairs, dist2, second2, count = got_matches(d1, [a for a, _ in sizes], d2, [b for _, b in sizes], max_matches=mm, **full)
        assert pairs.shape == (len(sizes), mm, 2) and dist2.shape == (len(sizes), mm) and second2.shape == dist2.shape
        for i, (a, b) in enumerate(sizes):
            wp, wd, ws, wc = sr.match_l2(d1[i, :a], d2[i, :b], max_matches=mm, **full)
            assert count[i] == wc and np.array_equal(pairs[i], wp) and np.array_equal(dist2[i], wd) and np.array_equal(second2[i], ws), \
                (kw, mm, a, b, count[i], wc)
        if mm == 700 and not full["cross_check"] and full["ratio"] is None and full["max_distance2"] is None:
            assert list(count) == [a if b else 0 for a, b in sizes]
            assert dist2[10, 0] == 0 and second2[10, 0] == 0                               # the duplicated rows
    alone = got_matches(d1[10:11], [513], d2[10:11], [600], max_matches=700, **full)
    assert all(np.array_equal(alone[k][0], (pairs, dist2, second2, count)[k][10]) for k in range(4))


@pytest.mark.gpu
def test_matcher_on_the_features_of_a_view_pair():
    a, b = sc.restated("roll10_a_ch1"), sc.restated("roll10_b_ch1")
    da, db = a["desc"][None], b["desc"][None]                                             # the restated descriptors: exact inputs
    for kw in (dict(ratio=0.75), dict(ratio=None, cross_check=True), dict(ratio=0.9, cross_check=True, max_distance2=60000)):
        got = got_matches(da, [a["count"]], db, [b["count"]], max_matches=sc.MAX_MATCHES, **kw)
        want = sr.match_l2(a["desc"][:a["count"]], b["desc"][:b["count"]], max_matches=sc.MAX_MATCHES, **kw)
        assert want[3] > 40 and all(np.array_equal(got[k][0], want[k]) for k in range(4)), kw


def _close(got, want, what, tol=1e-9):
    assert (np.abs(got - want) <= tol * (1 + np.abs(want))).all(), (what, float(np.abs(got - want).max()))


@pytest.mark.gpu
def test_poses_from_sift_on_the_view_pairs():
    names = [p[0] for p in fc.PAIRS]
    bgr = [fc.pose_frames(n) for n in names]
    rgb1, rgb2 = (np.stack([f[i][..., ::-1] for f in bgr]) for i in (0, 1))               # the reference's frames are R, G, B
    kw = dict(max_matches=sc.MAX_MATCHES, max_features=sc.MAX_FEATURES, hypotheses=fc.HYPOTHESES, seed=fc.SEED)
    R, T, mask, ok = camera_position.estimate_camera_poses_from_SIFT(rgb1, rgb2, fc.K, fc.BASELINE, **kw)
    assert R.shape == (3, 3, 3) and T.shape == (3, 3, 1) and mask.shape == (3, sc.MAX_MATCHES) and mask.dtype == np.uint8 and ok.all()
    for f, name in enumerate(names):
        x2d, want = sc.restated_chain(name)
        n = int(np.isfinite(x2d[0, :, 0]).sum())
        assert want["success"][0]
        _close(R[f], want["R"][0], (name, "R"))
        _close(T[f, :, 0], want["t"][0], (name, "T"))
        Rt, tt = fc.pair_pose(name)
        e = fc.pose_errors(R[f], T[f], Rt, tt)
        print(name, "rotation %.3f deg, direction %.3f deg" % e, "pose inliers", int(mask[f].sum()), "of", n)
        assert e[0] <= sc.ROT_BOUND_DEG and e[1] <= sc.DIR_BOUND_DEG
        assert abs(np.linalg.norm(T[f]) - fc.BASELINE) <= 1e-12
        # the clip's frame f is bitwise the single call with group_offset = f; pts are the restated matches
        Rf, Tf, p1, p2, mf = camera_position.estimate_camera_pose_from_SIFT(rgb1[f], rgb2[f], fc.K, fc.BASELINE, group_offset=f, **kw)
        assert Tf.shape == (3, 1) and np.array_equal(Rf, R[f]) and np.array_equal(Tf, T[f]) and np.array_equal(mf, mask[f, :n])
        assert p1.shape == (n, 2) and np.array_equal(p1, x2d[0, :n]) and np.array_equal(p2, x2d[1, :n]) and not mask[f, n:].any()
    # float frames in [0, 1] (the reference's other input) and device tensors give the same bits
    as_float = lambda a: torch.from_numpy((a.astype(np.float32) + 0.5) / 255.0).cuda()     # noqa: E731  (.byte() truncates back to a)
    Rd, Td, md, okd = camera_position.estimate_camera_poses_from_SIFT(as_float(rgb1), as_float(rgb2), fc.K, fc.BASELINE, **kw)
    assert np.array_equal(Rd, R) and np.array_equal(Td, T) and np.array_equal(md, mask) and np.array_equal(okd, ok)


@pytest.mark.gpu
def test_too_few_matches_and_the_bbox_region():
    flat = np.full((fc.H, fc.W, 3), 90, np.uint8)                                          # no keypoints, no matches
    with pytest.raises(ValueError, match="too few"):
        camera_position.estimate_camera_pose_from_SIFT(flat, flat, fc.K, fc.BASELINE)
    R, T, m = camera_position.estimate_pose_from_bbox_region(flat, flat, [0, 0, fc.W, fc.H], [0, 0, fc.W, fc.H], fc.K, fc.BASELINE)
    assert np.array_equal(R, np.eye(3)) and np.array_equal(T, np.zeros((3, 1))) and m is None
    name = fc.PAIRS[0][0]
    a, b = (f[..., ::-1] for f in fc.pose_frames(name))
    kw = dict(max_matches=sc.MAX_MATCHES, max_features=sc.MAX_FEATURES, hypotheses=fc.HYPOTHESES, seed=fc.SEED)
    # the whole frame as boxes (fractions are truncated as the reference's crop truncates them): the full-frame pose
    R, T, m = camera_position.estimate_pose_from_bbox_region(a, b, [0.4, 0.9, fc.W + 0.5, fc.H], [0, 0, fc.W, fc.H + 0.7], fc.K, fc.BASELINE, **kw)
    R0, T0, _, _, m0 = camera_position.estimate_camera_pose_from_SIFT(a, b, fc.K, fc.BASELINE, **kw)
    assert np.array_equal(R, R0) and np.array_equal(T, T0) and np.array_equal(m, m0)
    # boxes: only keypoints inside them are matched, in full-frame coordinates
    bl, br = [40, 30, 300, 220], [20, 20, 310, 230]
    R, T, m = camera_position.estimate_pose_from_bbox_region(a, b, bl, br, fc.K, fc.BASELINE, **kw)
    fa = sr.sift_features(np.ascontiguousarray(a[..., ::-1]), sc.MAX_FEATURES, roi=bl)
    fb = sr.sift_features(np.ascontiguousarray(b[..., ::-1]), sc.MAX_FEATURES, roi=br)
    want = sr.match_l2(fa["desc"][:fa["count"]], fb["desc"][:fb["count"]], 0.75, max_matches=sc.MAX_MATCHES)
    assert R.shape == (3, 3) and T.shape == (3, 1) and m.shape == (int(want[3]),) and want[3] >= 5
    assert abs(np.linalg.norm(T) - fc.BASELINE) <= 1e-12
    # a box without texture in it: the defaults
    R, T, m = camera_position.estimate_pose_from_bbox_region(a, b, [0, 0, 12, 12], br, fc.K, fc.BASELINE, **kw)
    assert np.array_equal(R, np.eye(3)) and not T.any() and m is None


@pytest.mark.gpu
def test_bad_arguments_raise_before_a_launch():
    frames = dev(sc.frames()["small_40x36"][None])
    for bad in (dict(max_features=0), dict(max_features=4097), dict(octaves=-1), dict(octaves=9)):
        with pytest.raises(_lib.SkimiError):
            geometry.sift_features(frames, **bad)
    with pytest.raises(_lib.SkimiError):
        geometry.sift_features(frames.cpu())
    with pytest.raises(_lib.SkimiError):
        geometry.sift_features(frames.float())
    with pytest.raises(_lib.SkimiError):
        geometry.sift_features(frames, roi=torch.zeros(1, 4, dtype=torch.float64))
    with pytest.raises(ValueError):
        geometry.sift_features(frames, roi=torch.zeros(2, 4, dtype=torch.float64).cuda())
    with pytest.raises(ValueError):
        geometry.sift_features(dev(np.zeros((1, 20, 20, 2), np.uint8)))
    d, n = torch.zeros(2, 10, 128, dtype=torch.uint8).cuda(), torch.zeros(2, dtype=torch.int32).cuda()
    for bad in (dict(max_matches=0), dict(max_matches=4097), dict(ratio=float("nan"))):
        with pytest.raises(_lib.SkimiError):
            geometry.match_l2(d, n, d, n, **bad)
    with pytest.raises(ValueError):
        geometry.match_l2(d, n, d[:1], n)
    with pytest.raises(ValueError):
        geometry.match_l2(d, n[:1], d, n)
    with pytest.raises(ValueError):
        geometry.match_l2(d.int(), n, d.int(), n)
    with pytest.raises(ValueError):
        geometry.match_l2(d[..., :64], n, d[..., :64], n)
    with pytest.raises(_lib.SkimiError):
        geometry.match_l2(d.cpu(), n, d, n)
    torch.cuda.synchronize()
