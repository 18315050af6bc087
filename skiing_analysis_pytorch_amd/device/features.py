"""ORB-style image features of whole frames and brute-force Hamming matching (csrc/features.hip; C-ABI:
skimi_orb_workspace_bytes, skimi_orb_features, skimi_match_hamming): camera_position.py:181-226
(estimate_camera_pose_from_ORB = cv2.ORB_create + cv2.BFMatcher(NORM_HAMMING, crossCheck=True)) under the project's own rules,
not OpenCV's; the reference's names are the package's camera_position.py; rules: include/skimi.h, DESIGN §2 "Image features".

Frames are uint8 [F, H, W, ch] or [C, F, H, W, ch] device tensors as device/chessboard.py takes them; every result carries the
frames' leading axes.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch

from .._args import descriptor_sets, f64, feature_frames, i32, workspace
from .._lib import check, current_stream, lib, ptr

ORB_MAX_LEVELS, ORB_MAX_FEATURES, ORB_BORDER = 8, 4096, 16
ORB_PATTERN_SEED = 0x534B494D494F5242
# round(2^14 cos / sin(2 pi k / 32)): SKIMI_ORB_COS, SKIMI_ORB_SIN of include/skimi.h
ORB_COS = (16384, 16069, 15137, 13623, 11585, 9102, 6270, 3196, 0, -3196, -6270, -9102, -11585, -13623, -15137, -16069, -16384, -16069,
           -15137, -13623, -11585, -9102, -6270, -3196, 0, 3196, 6270, 9102, 11585, 13623, 15137, 16069)
ORB_SIN = ORB_COS[24:] + ORB_COS[:24]


class OrbFeatures(NamedTuple):
    """orb_features' outputs (device tensors; M = max_features, L = levels)."""
    xy: torch.Tensor            # float64 [..., M, 2]: (x, y) in level-0 pixels; -1 behind the last keypoint
    xy_level: torch.Tensor      # int32 [..., M, 2]: the pixel in its level; levels in order, pixel order inside a level
    level: torch.Tensor         # int32 [..., M]; -1 behind the last keypoint
    direction: torch.Tensor     # int32 [..., M]: k of the angle 2 pi k / 32; -1 behind the last keypoint
    score: torch.Tensor         # int32 [..., M]: the FAST score s
    harris: torch.Tensor        # int64 [..., M]: the Harris response h
    desc: torch.Tensor          # int32 [..., M, 8]: 256 bits, bit i in word i / 32 at position i % 32
    count: torch.Tensor         # int32 [...]: the frame's keypoints (<= M)
    level_count: torch.Tensor   # int32 [..., L]: the candidates of every level, uncapped


class HammingMatches(NamedTuple):
    """match_hamming's outputs (int32 device tensors)."""
    pairs: torch.Tensor         # [..., max_matches, 2]: (query, train) by (distance, query); -1 behind the last pair
    dist: torch.Tensor          # [..., max_matches]: the Hamming distance; -1 behind the last pair
    count: torch.Tensor         # [...]: the pairs written


def _splitmix64(s):
    s = (s + 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
    z = s
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
    return s, z ^ (z >> 31)


def orb_pattern() -> np.ndarray:
    """The [32, 256, 4] int8 table of rule 7: (ax, ay, bx, by) of every bit for every direction, in Python integers."""
    s, base, seen = ORB_PATTERN_SEED, [], set()
    while len(base) < 256:
        v = []
        for _ in range(4):
            s, z = _splitmix64(s)
            v.append(z % 27 - 13)
        v = tuple(v)
        if v[0] * v[0] + v[1] * v[1] > 169 or v[2] * v[2] + v[3] * v[3] > 169 or v[:2] == v[2:] or v in seen:
            continue
        seen.add(v)
        base.append(v)
    tab = np.zeros((32, 256, 4), dtype=np.int8)
    for k in range(32):
        c, sn = ORB_COS[k], ORB_SIN[k]
        for i, (ax, ay, bx, by) in enumerate(base):
            tab[k, i] = ((ax * c - ay * sn + 8192) >> 14, (ax * sn + ay * c + 8192) >> 14,
                         (bx * c - by * sn + 8192) >> 14, (bx * sn + by * c + 8192) >> 14)
    return tab


_pattern_host = None
_pattern_dev = {}


def _pattern_on(dev):
    """the table, built once and uploaded once per device"""
    global _pattern_host
    if dev not in _pattern_dev:
        if _pattern_host is None:
            _pattern_host = torch.from_numpy(orb_pattern())
        _pattern_dev[dev] = _pattern_host.to(dev).contiguous()
    return _pattern_dev[dev]


def orb_features(frames: torch.Tensor, max_features: int = 500, levels: int = 8, threshold: int = 20, roi=None) -> OrbFeatures:
    """Oriented FAST keypoints with 256-bit rotated binary descriptors of every frame: a (5/6)^l pyramid of `levels` levels,
    the FAST-9 score s (the largest threshold at which the segment test passes) > threshold, 3 x 3 non-maximum suppression,
    the max_features best by an integer Harris response under per-level quotas, the direction from the intensity centroid
    as one of 32 integer angles, and the descriptor on a 5 x 5 blurred level.  roi [..., 4] (device; x1, y1, x2, y2 in level-0
    pixels, half-open) keeps only the keypoints inside a frame's box.  All integer: bitwise reproducible, and a frame gives
    the same bits alone and in a batch.  Nothing is read back."""
    fr, N, lead, box = feature_frames("orb_features", frames, roi)
    H, W, ch = (int(s) for s in fr.shape[2:])
    M, L, dev = int(max_features), int(levels), fr.device
    nws = int(lib().skimi_orb_workspace_bytes(N, H, W, L))
    xy, xyl = f64(dev, *lead, max(M, 0), 2), i32(dev, *lead, max(M, 0), 2)
    lvl, dirn, score = i32(dev, *lead, max(M, 0)), i32(dev, *lead, max(M, 0)), i32(dev, *lead, max(M, 0))
    har = torch.empty((*lead, max(M, 0)), dtype=torch.int64, device=dev)
    desc, count, lcount = i32(dev, *lead, max(M, 0), 8), i32(dev, *lead), i32(dev, *lead, max(L, 0))
    ws = workspace(dev, nws, at_least=16)
    check(lib().skimi_orb_features(ptr(fr), N, H, W, ch, L, int(threshold), M, ptr(box), ptr(_pattern_on(dev)), ptr(xyl), ptr(xy),
                                   ptr(lvl), ptr(dirn), ptr(score), ptr(har), ptr(desc), ptr(count), ptr(lcount), ptr(ws), nws,
                                   current_stream()), "skimi_orb_features")
    return OrbFeatures(xy, xyl, lvl, dirn, score, har, desc, count, lcount)


def match_hamming(d1: torch.Tensor, n1: torch.Tensor, d2: torch.Tensor, n2: torch.Tensor, cross_check: bool = True, ratio=None,
                  max_distance=None, max_matches: int = 1000) -> HammingMatches:
    """Brute-force Hamming matching of descriptor sets d1 [..., M1, 8] (query) and d2 [..., M2, 8] (train), int32 device
    tensors under common leading axes, of which the first n1 [...] and n2 [...] (device) rows count.  Each query's nearest
    train descriptor (ties to the smaller index); cross_check keeps it iff the train's nearest query is that query; ratio
    = r keeps it iff d_best < r d_second in float64 (a lone train descriptor fails); max_distance bounds d_best.  The kept
    pairs by (distance, query), the first max_matches of them: sorted(matches, key=distance)[:max_matches] of the
    reference.  One launch, nothing is read back."""
    lead, B, a, na, b, nb = descriptor_sets("match_hamming", d1, n1, d2, n2, 8, torch.int32, convert=True)
    dev, mm = d1.device, int(max_matches)
    pairs, dist, count = i32(dev, *lead, max(mm, 0), 2), i32(dev, *lead, max(mm, 0)), i32(dev, *lead)
    check(lib().skimi_match_hamming(ptr(a), ptr(na), int(d1.shape[-2]), ptr(b), ptr(nb), int(d2.shape[-2]), B, int(bool(cross_check)),
                                    -1.0 if ratio is None else float(ratio), -1 if max_distance is None else int(max_distance), mm,
                                    ptr(pairs), ptr(dist), ptr(count), current_stream()), "skimi_match_hamming")
    return HammingMatches(pairs, dist, count)
