"""GPU: the image features and the Hamming matcher (csrc/features.hip: orb_gray_kernel, orb_shrink_kernel, orb_blur_kernel,
orb_fast_kernel, orb_count_kernel, orb_write_kernel, orb_harris_kernel, orb_select_kernel, orb_describe_kernel, match_hamming_kernel;
geometry.orb_features, geometry.match_hamming, camera_position.estimate_camera_pose(s)_from_ORB) against the restatement
tests/features_restated.py on the frames of tests/features_cases.py.

Bounds: every stage is integer, so xy_level, level, direction, score, harris, desc, count, level_count, pairs, dist are
bitwise equal; xy is one float64 expression, within 1e-9 (1 + |x|).  The pose: R, T within 1e-9 (1 + |x|), the project's
float64 tolerance, of tests/essential_restated.py fed with the restated matches; against the truth within
features_cases.ROT_BOUND_DEG, DIR_BOUND_DEG."""
import numpy as np
import pytest
import torch

import features_cases as fc
import features_restated as fr
from skiing_analysis_pytorch_amd import _lib, camera_position, geometry

dev = lambda a: torch.from_numpy(np.array(a)).cuda()   # noqa: E731  (a copy: the cached frames are read-only)
INT_FIELDS = ("xy_level", "level", "direction", "score", "harris", "desc", "count", "level_count")
NAMES = sorted(fc.frames())


def got_features(frames, *a, **kw):
    r = geometry.orb_features(dev(frames), *a, **kw)
    assert r.xy.dtype == torch.float64 and r.harris.dtype == torch.int64 and r.desc.dtype == torch.int32
    return {k: getattr(r, k).cpu().numpy() for k in r._fields}


def same_features(got, want, what):
    for k in INT_FIELDS:
        assert np.array_equal(got[k], want[k]), (what, k, got["count"], want["count"], got["level_count"], want["level_count"])
    assert (np.abs(got["xy"] - want["xy"]) <= 1e-9 * (1 + np.abs(want["xy"]))).all(), what


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_features_are_bitwise_the_restatement(name):
    got = got_features(fc.frames()[name][None], fc.MAX_FEATURES)
    want = fc.restated(name)
    assert got["xy"].shape == (1, fc.MAX_FEATURES, 2) and got["desc"].shape == (1, fc.MAX_FEATURES, 8) and got["level_count"].shape == (1, 8)
    same_features({k: v[0] for k, v in got.items()}, want, name)
    print(name, "count", got["count"][0], "levels", got["level_count"][0])
    if name in ("constant", "small_30x30"):
        assert got["count"][0] == 0
    if name in ("noise", "tiled"):
        assert (got["level_count"][0, :5] > np.array(fr.quotas(fc.MAX_FEATURES, 8))[:5]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [dict(max_features=37, levels=3, threshold=35), dict(max_features=4096, levels=1, threshold=5),
                                dict(max_features=1, levels=8, threshold=20), dict(max_features=1000, levels=5, threshold=0)])
def test_other_quotas_levels_and_thresholds(kw):
    for name in ("crop_317x211", "tiled"):
        got = got_features(fc.frames()[name][None], **kw)
        same_features({k: v[0] for k, v in got.items()}, fr.orb_features(fc.frames()[name], **kw), (name, kw))


@pytest.mark.gpu
def test_a_batch_is_bitwise_its_frames_alone_and_a_rerun():
    clip = np.stack([np.stack(fc.view_pair(p[0])) for p in fc.PAIRS])[..., None]          # [3, 2, H, W, 1]
    clip = np.ascontiguousarray(clip.transpose(1, 0, 2, 3, 4))                            # [C = 2, F = 3, H, W, 1]
    batch, again = got_features(clip, 300), got_features(clip, 300)
    assert batch["xy"].shape == (2, 3, 300, 2) and batch["count"].shape == (2, 3) and batch["level_count"].shape == (2, 3, 8)
    for k in batch:
        assert np.array_equal(batch[k], again[k]), ("rerun", k)
    for c in range(2):
        for f in range(3):
            alone = got_features(clip[c, f][None], 300)
            for k in batch:
                assert np.array_equal(batch[k][c, f], alone[k][0]), (c, f, k)
    flat = got_features(clip.reshape(6, fc.H, fc.W, 1), 300)
    for k in batch:
        assert np.array_equal(batch[k].reshape(flat[k].shape), flat[k]), ("four axes", k)


@pytest.mark.gpu
def test_roi_keeps_the_keypoints_of_a_box():
    name = "roll-20_in_a_ch3"
    frame = fc.frames()[name]
    boxes = np.array([[60.0, 40.5, 250.0, 200.0], [0.0, 0.0, fc.W, fc.H], [100.0, 50.0, np.nan, 200.0], [200.0, 100.0, 100.0, 200.0],
                      [-np.inf, -np.inf, np.inf, 120.0]])
    got = got_features(np.stack([frame] * len(boxes)), fc.MAX_FEATURES, roi=dev(boxes))
    for i, box in enumerate(boxes):
        want = fr.orb_features(frame, fc.MAX_FEATURES, roi=box)
        same_features({k: v[i] for k, v in got.items()}, want, (name, i))
        n = got["count"][i]
        xy = got["xy"][i, :n]
        assert ((xy[:, 0] >= box[0]) & (xy[:, 0] < box[2]) & (xy[:, 1] >= box[1]) & (xy[:, 1] < box[3])).all()
    assert got["count"][0] > 50 and got["count"][2] == 0 and got["count"][3] == 0 and got["count"][4] > 50
    same_features({k: v[1] for k, v in got.items()}, fc.restated(name), "the whole frame as a box")


def got_matches(d1, n1, d2, n2, **kw):
    r = geometry.match_hamming(dev(d1), dev(np.asarray(n1, np.int32)), dev(d2), dev(np.asarray(n2, np.int32)), **kw)
    assert all(t.dtype == torch.int32 for t in r)
    return [t.cpu().numpy() for t in r]


def _sets(rng, n, pad):
    """n descriptors a few bits from 16 prototypes (ties everywhere), two of them equal, in `pad` rows of noise"""
    base = rng.integers(-2 ** 31, 2 ** 31, (16, 8), dtype=np.int64).astype(np.int32)
    d = rng.integers(-2 ** 31, 2 ** 31, (pad, 8), dtype=np.int64).astype(np.int32)
    if n:
        d[:n] = base[rng.integers(0, 16, n)] ^ (np.int32(1) << rng.integers(0, 31, (n, 8)).astype(np.int32))
    if n > 4:
        d[3] = d[1]
    return d


MATCH_MODES = [dict(cross_check=True), dict(cross_check=False, ratio=0.8), dict(cross_check=False, max_distance=12),
               dict(cross_check=True, ratio=0.95, max_distance=40), dict(cross_check=False)]


@pytest.mark.gpu
@pytest.mark.parametrize("kw", MATCH_MODES)
def test_matcher_is_bitwise_the_restatement(kw):
    """set sizes around the wave (63, 65), the workgroup (257) and the staging buffer (513, 600), empty sets, a lone train
    descriptor; one call for all pairs of sets, the rows behind n1, n2 hold noise"""
    rng = np.random.default_rng(17)
    sizes = [(0, 5), (5, 0), (1, 1), (1, 63), (63, 65), (65, 63), (257, 65), (40, 257), (513, 600), (640, 511), (2, 1)]
    M1, M2 = 640, 600
    d1 = np.stack([_sets(rng, a, M1) for a, _ in sizes])
    d2 = np.stack([_sets(rng, b, M2) for _, b in sizes])
    full = dict(dict(cross_check=True, ratio=None, max_distance=None), **kw)
    for mm in (9, 700):
        pairs, dist, count = got_matches(d1, [a for a, _ in sizes], d2, [b for _, b in sizes], max_matches=mm, **kw)
        assert pairs.shape == (len(sizes), mm, 2) and dist.shape == (len(sizes), mm) and count.shape == (len(sizes),)
        for i, (a, b) in enumerate(sizes):
            wp, wd, wc = fr.match_hamming(d1[i, :a], d2[i, :b], max_matches=mm, **full)
            assert count[i] == wc and np.array_equal(pairs[i], wp) and np.array_equal(dist[i], wd), (kw, mm, a, b)
        if mm == 700 and not full["cross_check"] and full["ratio"] is None and full["max_distance"] is None:
            assert list(count) == [a if b else 0 for a, b in sizes]
    alone = got_matches(d1[8:9], [513], d2[8:9], [600], max_matches=700, **kw)
    assert np.array_equal(alone[0][0], pairs[8]) and np.array_equal(alone[1][0], dist[8]) and alone[2][0] == count[8]


@pytest.mark.gpu
def test_matcher_on_the_features_of_a_view_pair():
    a, b = fc.restated("roll10_a_ch1"), fc.restated("roll10_b_ch1")
    fa, fb = (geometry.orb_features(dev(fc.frames()[n][None]), fc.MAX_FEATURES) for n in ("roll10_a_ch1", "roll10_b_ch1"))
    for kw in (dict(cross_check=True), dict(cross_check=False, ratio=0.75)):
        m = geometry.match_hamming(fa.desc, fa.count, fb.desc, fb.count, max_matches=fc.MAX_MATCHES, **kw)
        full = dict(dict(cross_check=True, ratio=None, max_distance=None), **kw)
        wp, wd, wc = fr.match_hamming(a["desc"][:a["count"]], b["desc"][:b["count"]], max_matches=fc.MAX_MATCHES, **full)
        assert int(m.count[0]) == wc and wc > 100 and np.array_equal(m.pairs[0].cpu().numpy(), wp) and np.array_equal(m.dist[0].cpu().numpy(), wd)


def _close(got, want, what, tol=1e-9):
    assert (np.abs(got - want) <= tol * (1 + np.abs(want))).all(), (what, float(np.abs(got - want).max()))


@pytest.mark.gpu
def test_poses_from_orb_on_the_view_pairs():
    names = [p[0] for p in fc.PAIRS]
    bgr = [fc.pose_frames(n) for n in names]
    rgb1, rgb2 = (np.stack([f[i][..., ::-1] for f in bgr]) for i in (0, 1))               # the reference's frames are R, G, B
    kw = dict(max_matches=fc.MAX_MATCHES, max_features=fc.MAX_FEATURES, hypotheses=fc.HYPOTHESES, seed=fc.SEED)
    R, T, mask, ok = camera_position.estimate_camera_poses_from_ORB(rgb1, rgb2, fc.K, fc.BASELINE, **kw)
    assert R.shape == (3, 3, 3) and T.shape == (3, 3, 1) and mask.shape == (3, fc.MAX_MATCHES) and mask.dtype == np.uint8 and ok.all()
    for f, name in enumerate(names):
        x2d, want = fc.restated_chain(name)
        assert want["success"][0]
        _close(R[f], want["R"][0], (name, "R"))
        _close(T[f, :, 0], want["t"][0], (name, "T"))
        Rt, tt = fc.pair_pose(name)
        e = fc.pose_errors(R[f], T[f], Rt, tt)
        print(name, "rotation %.3f deg, direction %.3f deg" % e, "pose inliers", int(mask[f].sum()), "of", int(np.isfinite(x2d[0, :, 0]).sum()))
        assert e[0] <= fc.ROT_BOUND_DEG and e[1] <= fc.DIR_BOUND_DEG
        assert abs(np.linalg.norm(T[f]) - fc.BASELINE) <= 1e-12
        # the clip's frame f is bitwise the single call with group_offset = f
        Rf, Tf, mf = camera_position.estimate_camera_pose_from_ORB(rgb1[f], rgb2[f], fc.K, fc.BASELINE, group_offset=f, **kw)
        assert Tf.shape == (3, 1) and np.array_equal(Rf, R[f]) and np.array_equal(Tf, T[f]) and np.array_equal(mf, mask[f])
    # float frames in [0, 1] (the reference's other input) and device tensors give the same bits
    as_float = lambda a: torch.from_numpy((a.astype(np.float32) + 0.5) / 255.0).cuda()     # noqa: E731  (.byte() truncates back to a)
    Rd, Td, md, okd = camera_position.estimate_camera_poses_from_ORB(as_float(rgb1), as_float(rgb2), fc.K, fc.BASELINE, **kw)
    assert np.array_equal(Rd, R) and np.array_equal(Td, T) and np.array_equal(md, mask) and np.array_equal(okd, ok)
    flat = np.full((fc.H, fc.W, 3), 90, np.uint8)                                          # no keypoints, no matches, no pose
    assert camera_position.estimate_camera_pose_from_ORB(flat, flat, fc.K, fc.BASELINE, **kw) == (None, None, None)


@pytest.mark.gpu
def test_bad_arguments_raise_before_a_launch():
    frames = dev(fc.frames()["small_40x36"][None])
    for bad in (dict(max_features=0), dict(max_features=4097), dict(levels=0), dict(levels=9), dict(threshold=-1), dict(threshold=255)):
        with pytest.raises(_lib.SkimiError):
            geometry.orb_features(frames, **bad)
    with pytest.raises(_lib.SkimiError):
        geometry.orb_features(frames.cpu())
    with pytest.raises(_lib.SkimiError):
        geometry.orb_features(frames, roi=torch.zeros(1, 4, dtype=torch.float64))
    with pytest.raises(ValueError):
        geometry.orb_features(frames, roi=torch.zeros(2, 4, dtype=torch.float64).cuda())
    d, n = torch.zeros(2, 10, 8, dtype=torch.int32).cuda(), torch.zeros(2, dtype=torch.int32).cuda()
    for bad in (dict(max_matches=0), dict(max_matches=4097), dict(ratio=float("nan")), dict(max_distance=257)):
        with pytest.raises(_lib.SkimiError):
            geometry.match_hamming(d, n, d, n, **bad)
    with pytest.raises(ValueError):
        geometry.match_hamming(d, n, d[:1], n)
    with pytest.raises(ValueError):
        geometry.match_hamming(d, n[:1], d, n)
    with pytest.raises(_lib.SkimiError):
        geometry.match_hamming(d.cpu(), n, d, n)
    torch.cuda.synchronize()
