"""CPU: the image-feature rules themselves (tests/features_restated.py, the tables of include/skimi.h and of
device/features.py) against their literal definitions, and the restated chain end to end on the view pairs of
tests/features_cases.py: the match-quality condition and the truth bounds of the pose."""
import re
from pathlib import Path

import numpy as np
import pytest

import features_cases as fc
import features_restated as fr

ROOT = Path(__file__).resolve().parent.parent


def _header_table(name):
    text = (ROOT / "include" / "skimi.h").read_text()
    body = re.search(rf"#define {name}\s*\\\n(.*?)\}}", text, flags=re.S).group(1)
    return [int(v) for v in re.findall(r"-?\d+", body)]


def test_fast_score_is_the_largest_passing_threshold():
    """s > t exactly when the segment test passes at t: the largest passing threshold is s - 1 (none passes: s = 0)"""
    rng = np.random.default_rng(0)
    n = 2 * fr.BORDER + 8
    blobs = rng.integers(0, 3, (n // 4 + 1, n // 4 + 1)).repeat(4, axis=0).repeat(4, axis=1)[:n, :n] * 60 + 40
    images = [rng.integers(0, 256, (n, n)), blobs + rng.integers(-3, 4, (n, n)), rng.integers(100, 110, (n, n))]
    corners = 0
    for img in images:
        s = fr.fast_score(img.astype(np.int64))
        assert (s[:fr.BORDER] == 0).all() and (s[:, :fr.BORDER] == 0).all() and (s[-fr.BORDER:] == 0).all() and (s[:, -fr.BORDER:] == 0).all()
        for y in range(fr.BORDER, n - fr.BORDER):
            for x in range(fr.BORDER, n - fr.BORDER):
                lit = fr.fast_score_literal(img[y - 3:y + 4, x - 3:x + 4])
                assert lit == s[y, x] - 1, (x, y, lit, s[y, x])
                corners += s[y, x] > 20
    assert corners >= 10


def test_tables_and_rotated_patterns():
    assert _header_table("SKIMI_ORB_COS") == fr.COS and _header_table("SKIMI_ORB_SIN") == fr.SIN
    from skiing_analysis_pytorch_amd.device import features as df
    assert list(df.ORB_COS) == fr.COS and list(df.ORB_SIN) == fr.SIN and df.ORB_PATTERN_SEED == fr.PATTERN_SEED
    assert f"{fr.PATTERN_SEED:#018X}".replace("0X", "0x") + "ULL" in (ROOT / "include" / "skimi.h").read_text()
    tab = fr.rotated_patterns()
    assert tab.shape == (32, 256, 4)
    for h in (0, 2):
        assert ((tab[:, :, h] ** 2 + tab[:, :, h + 1] ** 2) <= 14 * 14).all()
    assert (np.abs(tab) <= fr.BORDER - 2).all()          # a keypoint's samples and their 5 x 5 blur stay inside the level
    base = fr.base_pattern()
    assert np.array_equal(tab[0], base) and (np.abs(base) <= 13).all()
    assert ((base[:, 0] ** 2 + base[:, 1] ** 2) <= 169).all() and ((base[:, 2] ** 2 + base[:, 3] ** 2) <= 169).all()
    assert ((base[:, 0] != base[:, 2]) | (base[:, 1] != base[:, 3])).all()                  # the two points of a pair differ
    assert len({tuple(r) for r in base.tolist()}) == 256                                   # and no pair comes twice
    for k in range(32):                                                                    # in every direction too
        assert ((tab[k, :, 0] != tab[k, :, 2]) | (tab[k, :, 1] != tab[k, :, 3])).all(), k
    # a quarter turn of the pattern is exact: (x, y) -> (-y, x) for k -> k + 8
    for k in range(32):
        q = tab[(k + 8) % 32]
        assert np.array_equal(q[:, [0, 2]], -tab[k][:, [1, 3]]) and np.array_equal(q[:, [1, 3]], tab[k][:, [0, 2]]), k
    got = df.orb_pattern()
    assert got.dtype == np.int8 and np.array_equal(got.astype(np.int64), tab)


def test_level_sizes_and_quotas():
    assert [fr.level_size(320, l) for l in range(8)] == [320, 267, 222, 185, 154, 129, 107, 89]
    for M in (1, 7, 500, 4096):
        for L in range(1, 9):
            q = fr.quotas(M, L)
            assert sum(q) == M and min(q) >= 0 and all(q[l] >= q[l + 1] for l in range(L - 1))
    assert fr.quotas(500, 8) == [500 - sum(fr.quotas(500, 8)[1:])] + fr.quotas(500, 8)[1:]
    assert [fr.level_size(40, 1), fr.level_size(36, 1)] == [33, 30]          # small_40x36: only level 0 has room


def test_quarter_turn_shifts_directions_by_eight():
    """np.rot90 takes the pixel (x, y) of a W-wide frame to (y, W - 1 - x) and the angle k to k - 8: the same keypoints (where
    the raster tie rule of the suppression does not decide), the same descriptors"""
    img = fc.view_pair("roll10")[0]
    a = fr.orb_features(img, 4096, 1, 20)
    b = fr.orb_features(np.rot90(img).copy(), 4096, 1, 20)
    Wd = img.shape[1]
    na, nb = int(a["count"]), int(b["count"])
    assert na > 100 and nb > 100
    where = {(int(x), int(y)): i for i, (x, y) in enumerate(b["xy_level"][:nb])}
    same = 0
    s = fr.fast_score(fr.gray(img))
    for i, (x, y) in enumerate(a["xy_level"][:na]):
        j = where.get((int(y), Wd - 1 - int(x)))
        if j is None:                                    # only a tie with a neighbour can take a keypoint away
            assert (s[y - 1:y + 2, x - 1:x + 2] == s[y, x]).sum() >= 2, (x, y)
            continue
        same += 1
        assert a["score"][i] == b["score"][j] and a["harris"][i] == b["harris"][j]
        assert (a["direction"][i] - 8) % 32 == b["direction"][j]
        assert np.array_equal(a["desc"][i], b["desc"][j])
    assert same * 2 >= max(na, nb), (same, na, nb)


def _literal_matches(d1, d2, cross_check, ratio, max_distance, max_matches):
    dist = lambda a, b: sum(bin(int(x) ^ int(y)).count("1") for x, y in zip(a.view(np.uint32), b.view(np.uint32)))   # noqa: E731
    D = [[dist(a, b) for b in d2] for a in d1]
    out = []
    for i in range(len(d1)):
        if not len(d2):
            continue
        order = sorted(range(len(d2)), key=lambda j: D[i][j])                               # stable: the smaller index first
        j = order[0]
        if cross_check and min(range(len(d1)), key=lambda k: (D[k][j], k)) != i:
            continue
        if ratio is not None and (len(order) < 2 or not D[i][j] < ratio * D[i][order[1]]):    # the reference's len(m) == 2
            continue
        if max_distance is not None and D[i][j] > max_distance:
            continue
        out.append((D[i][j], i, j))
    out = sorted(out, key=lambda m: m[0])[:max_matches]                                     # the reference's sorted(...)[:max]
    return out


def _descriptors(rng, n, dup=0):
    d = rng.integers(-2 ** 31, 2 ** 31, (n, 8), dtype=np.int64).astype(np.int32)
    for _ in range(dup):
        if n >= 2:
            i, j = rng.integers(0, n, 2)
            d[i] = d[j]
    return d


@pytest.mark.parametrize("n1,n2", [(0, 5), (5, 0), (1, 1), (1, 63), (63, 65), (65, 63), (257, 65), (40, 257)])
@pytest.mark.parametrize("mode", ["cross", "ratio", "plain_maxdist", "cross_ratio"])
def test_matcher_against_the_literal_loops(n1, n2, mode):
    rng = np.random.default_rng(n1 * 1000 + n2)
    base = _descriptors(rng, 16)
    near = lambda n: base[rng.integers(0, 16, n)] ^ (np.int32(1) << rng.integers(0, 31, (n, 8)).astype(np.int32)) if n else _descriptors(rng, 0)   # noqa: E731
    d1, d2 = near(n1), near(n2)                          # few distinct distances: ties everywhere
    if n1 > 4:
        d1[3] = d1[1]
    if n2 > 4:
        d2[4] = d2[0]
    kw = dict(cross=dict(cross_check=True), ratio=dict(cross_check=False, ratio=0.8),
              plain_maxdist=dict(cross_check=False, max_distance=12), cross_ratio=dict(cross_check=True, ratio=0.95))[mode]
    kw = dict(dict(cross_check=True, ratio=None, max_distance=None), **kw)
    for mm in (7, 300):
        pairs, dist, count = fr.match_hamming(d1, d2, max_matches=mm, **kw)
        want = _literal_matches(d1, d2, kw["cross_check"], kw["ratio"], kw["max_distance"], mm)
        assert count == len(want)
        assert [(int(d), int(p[0]), int(p[1])) for d, p in zip(dist[:count], pairs[:count])] == want
        assert (pairs[count:] == -1).all() and (dist[count:] == -1).all()


def test_counting_sort_is_pythons_stable_sort():
    rng = np.random.default_rng(3)
    for n in (0, 1, 64, 1000):
        d = rng.integers(0, 257, n)
        assert list(fr.counting_sort_order(d)) == sorted(range(n), key=lambda i: d[i])


def test_edge_frames():
    assert fc.restated("constant")["count"] == 0 and fc.restated("small_30x30")["count"] == 0
    assert (fc.restated("small_30x30")["level_count"] == 0).all()
    small = fc.restated("small_40x36")
    assert small["level_count"][0] > 0 and (small["level_count"][1:] == 0).all()
    q = np.array(fr.quotas(fc.MAX_FEATURES, 8))
    for name in ("noise", "tiled"):
        r = fc.restated(name)
        assert (r["level_count"][:5] > q[:5]).all() and r["count"] == np.minimum(r["level_count"], q).sum(), (name, r["level_count"])
    t = fc.restated("tiled")                               # equal responses on both sides of the cut: the tie rule decides
    lv0 = t["level"] == 0
    cut = t["harris"][lv0].min()
    all0 = fr.orb_features(fc.frames()["tiled"], 4096, 1, 20)
    assert (all0["harris"][:all0["count"]] == cut).sum() > (t["harris"][lv0] == cut).sum()


@pytest.mark.parametrize("name", [p[0] for p in fc.PAIRS])
def test_restated_chain_pose_and_match_quality(name):
    R, t = fc.pair_pose(name)
    worst = [0.0, 0.0]
    for seed in fc.TRUTH_SEEDS:
        f1, f2 = fc.view_pair(name, seed)
        (pairs, dist, count), x2d = fc.chain_inputs(f1, f2)
        err = np.linalg.norm(fc.true_match(R, t, x2d[0, :count]) - x2d[1, :count], axis=1)
        assert count >= 100 and (err <= 3.0).sum() * 2 >= count, (name, seed, count, int((err <= 3.0).sum()))
        assert (np.diff(dist[:count]) >= 0).all()
        r = fc.chain_pose(x2d)
        assert r["success"][0]
        e = fc.pose_errors(r["R"][0], r["t"][0], R, t)
        print(name, seed, "matches", count, "within 3 px", int((err <= 3.0).sum()), "rotation %.3f deg, direction %.3f deg" % e)
        worst = [max(worst[0], e[0]), max(worst[1], e[1])]
        assert e[0] <= fc.ROT_BOUND_DEG and e[1] <= fc.DIR_BOUND_DEG
    assert worst[0] <= fc.MEASURED_ROT_DEG + 1e-3 and worst[1] <= fc.MEASURED_DIR_DEG + 1e-3   # the recorded worst values stand
    # the frames of the GPU comparison (the same scenes with colour noise) meet both conditions too
    x2d, r = fc.restated_chain(name)
    n = int(np.isfinite(x2d[0, :, 0]).sum())
    err = np.linalg.norm(fc.true_match(R, t, x2d[0, :n]) - x2d[1, :n], axis=1)
    e = fc.pose_errors(r["R"][0], r["t"][0], R, t)
    print(name, "comparison frames: matches", n, "within 3 px", int((err <= 3.0).sum()), "rotation %.3f deg, direction %.3f deg" % e)
    assert (err <= 3.0).sum() * 2 >= n and r["success"][0] and e[0] <= fc.ROT_BOUND_DEG and e[1] <= fc.DIR_BOUND_DEG
