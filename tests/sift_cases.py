"""Frames for the SIFT-style feature tests: the rendered view pairs, textures and edge frames of tests/features_cases.py plus
the sizes at which the scale space changes path.  The restated results are computed once and shared (tests/sift_restated.py,
tests/essential_restated.py).

Truth bounds of the end-to-end pose (features -> ratio-tested L2 matches -> essential_ransac), measured with the restatement on
the CPU over features_cases.PAIRS x TRUTH_SEEDS (tests/test_sift_cpu.py::test_restated_chain_pose_and_match_quality prints
them):
    worst rotation angle error            MEASURED_ROT_DEG
    worst translation-direction error     MEASURED_DIR_DEG
and the bounds are twice those, as for the ORB chain (3.342 and 11.297 degrees there).
"""
import functools

import numpy as np

import features_cases as fc
import sift_restated as sr

MAX_FEATURES, MAX_MATCHES, RATIO = 500, 256, 0.75
MAX_FEATURES_BLOBS = 200                  # the frame "blobs" has more keypoints: the selection runs
# (queries, train rows) of the matcher's sets: empty sets, a lone train row, around the wave and the query block (63, 65), the
# sort's span of a wave (257) and several chunks of everything (513, 600)
MATCH_SIZES = ((0, 5), (5, 0), (1, 1), (2, 1), (1, 2), (5, 63), (63, 65), (65, 63), (257, 65), (40, 257), (513, 600), (600, 513))
MATCH_PAD = 640
MATCH_MODES = (dict(ratio=None), dict(ratio=0.75), dict(ratio=1.0), dict(ratio=None, cross_check=True), dict(ratio=0.75, cross_check=True),
               dict(ratio=None, max_distance2=1200), dict(ratio=1.0, cross_check=True, max_distance2=1500))
MEASURED_ROT_DEG, MEASURED_DIR_DEG = 2.264, 9.344       # pair roll10 seed 3; pair roll-20_in seed 1
ROT_BOUND_DEG, DIR_BOUND_DEG = 2 * MEASURED_ROT_DEG, 2 * MEASURED_DIR_DEG
# the restated descriptor of a frame turned by 90 degrees (np.rot90: an exact resampling) against the original's: the worst
# difference of a byte over the keypoints found in both, measured by test_sift_cpu.py::test_rot90_descriptor
MEASURED_ROT90_LEVELS = 1                 # 126 keypoints of crop_317x211, two octaves; the test's bound is twice this


@functools.lru_cache(maxsize=None)
def frames():
    """name -> uint8 [h, w, ch]: the frames of the bitwise comparison"""
    src = fc.frames()
    out = {k: v for k, v in src.items() if "_ch" in k}               # the six 320 x 240 view frames, ch 1, 3, 4
    for k in ("crop_317x211", "constant", "noise", "tiled", "small_40x36"):
        out[k] = src[k]
    rng = np.random.default_rng(5)                                  # 5 x 5 blocks of noise: more keypoints than MAX_FEATURES_BLOBS
    out["blobs"] = np.kron(rng.integers(0, 256, (49, 65), dtype=np.uint8), np.ones((5, 5), np.uint8))[:fc.H, :fc.W, None]
    out["tiny_15x15"] = np.random.default_rng(6).integers(0, 256, (15, 15, 1), dtype=np.uint8)
    return out


def max_features_of(name):
    return MAX_FEATURES_BLOBS if name == "blobs" else MAX_FEATURES


@functools.lru_cache(maxsize=None)
def restated(name, max_features=MAX_FEATURES, octaves=None):
    return sr.sift_features(frames()[name], max_features, octaves)


def chain_inputs(f1, f2, max_features=MAX_FEATURES, max_matches=MAX_MATCHES, ratio=RATIO):
    """restated features of two frames -> (features, features, matches, x2d [2, max_matches, 2] NaN-padded)"""
    a, b = sr.sift_features(f1, max_features), sr.sift_features(f2, max_features)
    m = sr.match_l2(a["desc"][:a["count"]], b["desc"][:b["count"]], ratio, False, None, max_matches)
    pairs, count = m[0], m[3]
    x2d = np.full((2, max_matches, 2), np.nan)
    x2d[0, :count], x2d[1, :count] = a["xy"][pairs[:count, 0]], b["xy"][pairs[:count, 1]]
    return a, b, m, x2d


@functools.lru_cache(maxsize=None)
def restated_chain(name):
    """the restated chain on features_cases.pose_frames(name) as frame f of the clip: (x2d, the restated essential_ransac)"""
    *_, x2d = chain_inputs(*fc.pose_frames(name))
    return x2d, fc.chain_pose(x2d, [p[0] for p in fc.PAIRS].index(name))


def _set(rng, proto, n, pad):
    """n descriptors a few levels from 16 prototypes (near ties everywhere), two of them equal, in `pad` rows of noise"""
    d = rng.integers(0, 256, (pad, 128), dtype=np.uint8)
    if n:
        d[:n] = np.clip(proto[rng.integers(0, 16, n)].astype(np.int64) + rng.integers(-2, 3, (n, 128)), 0, 255).astype(np.uint8)
    if n > 4:
        d[3] = d[1]
    return d


@functools.lru_cache(maxsize=None)
def match_sets():
    """(d1, d2) uint8 [pairs, MATCH_PAD, 128]; where both sets have five rows, query 0 equals the train rows 1 and 3"""
    rng = np.random.default_rng(17)
    proto = rng.integers(0, 256, (16, 128), dtype=np.uint8)
    d1 = np.stack([_set(rng, proto, a, MATCH_PAD) for a, _ in MATCH_SIZES])
    d2 = np.stack([_set(rng, proto, b, MATCH_PAD) for _, b in MATCH_SIZES])
    for i, (a, b) in enumerate(MATCH_SIZES):
        if a > 4 and b > 4:
            d1[i, 0] = d2[i, 1]
    return d1, d2
