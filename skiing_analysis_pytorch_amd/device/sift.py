"""SIFT-style image features of whole frames and brute-force L2 matching with Lowe's ratio test (csrc/sift.hip; C-ABI:
skimi_sift_workspace_bytes, skimi_sift_features, skimi_match_l2): camera_position.py:120-178, 242-297
(estimate_camera_pose_from_SIFT, estimate_pose_from_bbox_region = cv2.SIFT_create + BFMatcher.knnMatch(k=2) + ratio test) under
the project's own rules, not OpenCV's: parity with cv2.SIFT_create is not pinned.  The reference's names are the package's
camera_position.py; rules: include/skimi.h, DESIGN §2 "Image features (SIFT-style)".

Frames are uint8 [F, H, W, ch] or [C, F, H, W, ch] device tensors as device/features.py takes them; every result carries the
frames' leading axes.
"""
from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np
import torch

from .._args import descriptor_sets, f64, feature_frames, i32, u8, workspace
from .._lib import check, current_stream, lib, ptr

SIFT_MAX_OCTAVES, SIFT_MAX_FEATURES, SIFT_MAX_CANDIDATES, SIFT_BORDER, SIFT_MIN_SIDE = 8, 4096, 32768, 5, 16
SIFT_INTERVALS, SIFT_SIGMA0, SIFT_MAX_RADIUS = 3, 1.6, 13
SIFT_RADII = (7, 5, 7, 8, 10, 13)               # SKIMI_SIFT_RADII: ceil(4 sigma) of the six blurs


class SiftFeatures(NamedTuple):
    """sift_features' outputs (device tensors; M = max_features, O = octaves)."""
    xy: torch.Tensor            # float64 [..., M, 2]: (x, y) in level-0 pixels; -1 behind the last keypoint
    xy_level: torch.Tensor      # int32 [..., M, 2]: the pixel in its octave after refinement; -1 behind the last keypoint
    octave: torch.Tensor        # int32 [..., M]; -1 behind the last keypoint
    layer: torch.Tensor         # int32 [..., M]: the DoG layer 1 .. 3 after refinement; -1 behind the last keypoint
    sigma: torch.Tensor         # float64 [..., M]: the scale in level-0 pixels; 0 behind the last keypoint
    response: torch.Tensor      # float64 [..., M]: the interpolated DoG value D(x^); 0 behind the last keypoint
    angle: torch.Tensor         # float64 [..., M]: radians in [0, 2 pi), from x towards y; -1 behind the last keypoint
    desc: torch.Tensor          # uint8 [..., M, 128]: entry (row 4 + column) 8 + orientation
    count: torch.Tensor         # int32 [...]: the frame's keypoints (<= M)
    octave_count: torch.Tensor  # int32 [..., O]: the candidates of every octave, uncapped


class L2Matches(NamedTuple):
    """match_l2's outputs (int32 device tensors)."""
    pairs: torch.Tensor         # [..., max_matches, 2]: (query, train) by (distance, query); -1 behind the last pair
    dist2: torch.Tensor         # [..., max_matches]: the squared distance to the nearest; -1 behind the last pair
    second2: torch.Tensor       # [..., max_matches]: the squared distance to the second nearest (-1: none, and behind)
    count: torch.Tensor         # [...]: the pairs written


def sift_sigmas():
    """the six blurs of an octave: layer 0 of octave 0 from the frame, then layer i from layer i - 1"""
    k = 2.0 ** (1.0 / SIFT_INTERVALS)
    return [math.sqrt(SIFT_SIGMA0 * SIFT_SIGMA0 - 0.25)] + [SIFT_SIGMA0 * k ** (i - 1) * math.sqrt(k * k - 1.0)
                                                              for i in range(1, SIFT_INTERVALS + 3)]


def sift_taps() -> np.ndarray:
    """The [6, 27] float32 table of rule 2: row i holds layer i's taps of radius ceil(4 sigma_i) around column 13, made in
    float64, normalised to sum 1 and then rounded; zero outside the radius."""
    tab = np.zeros((len(SIFT_RADII), 2 * SIFT_MAX_RADIUS + 1), dtype=np.float32)
    for i, s in enumerate(sift_sigmas()):
        r = int(math.ceil(4.0 * s))
        assert r == SIFT_RADII[i]
        x = np.arange(-r, r + 1, dtype=np.float64)
        g = np.exp(-(x * x) / (2.0 * s * s))
        tab[i, SIFT_MAX_RADIUS - r:SIFT_MAX_RADIUS + r + 1] = (g / g.sum()).astype(np.float32)
    return tab


def sift_octaves(H: int, W: int) -> int:
    """the octaves that keep min(W_o, H_o) >= 16, at most 8: sift_features' default"""
    n = 0
    while n < SIFT_MAX_OCTAVES and min(H, W) >= SIFT_MIN_SIDE:
        n, H, W = n + 1, (H + 1) // 2, (W + 1) // 2
    return n


_taps_host = None
_taps_dev = {}


def _taps_on(dev):
    """the table, built once and uploaded once per device"""
    global _taps_host
    if dev not in _taps_dev:
        if _taps_host is None:
            _taps_host = torch.from_numpy(sift_taps())
        _taps_dev[dev] = _taps_host.to(dev).contiguous()
    return _taps_dev[dev]


def sift_features(frames: torch.Tensor, max_features: int = 3000, octaves=None, roi=None) -> SiftFeatures:
    """Scale-space keypoints with 128-byte gradient-histogram descriptors of every frame: a float32 Gaussian scale space (3
    intervals an octave, sigma0 1.6, no doubled first octave; `octaves` defaults to those with a side of 16 or more), the
    26-neighbour extrema of the differences of Gaussians, a float64 quadratic refinement to sub-pixel, sub-scale positions
    with contrast and edge tests, the max_features of largest |response|, one orientation (36 bins, interpolated votes) and
    a 4 x 4 x 8 descriptor.  roi [..., 4] (device; x1, y1, x2, y2 in level-0 pixels, half-open) keeps only the keypoints
    inside a frame's box.  Bitwise reproducible, and a frame gives the same bits alone and in a batch.  Nothing is read
    back."""
    fr, N, lead, box = feature_frames("sift_features", frames, roi)
    H, W, ch = (int(s) for s in fr.shape[2:])
    M, dev = int(max_features), fr.device
    O = sift_octaves(H, W) if octaves is None else int(octaves)
    nws = int(lib().skimi_sift_workspace_bytes(N, H, W, O))
    m = max(M, 0)
    xy, xyl, octv, lay = f64(dev, *lead, m, 2), i32(dev, *lead, m, 2), i32(dev, *lead, m), i32(dev, *lead, m)
    sig, resp, ang = f64(dev, *lead, m), f64(dev, *lead, m), f64(dev, *lead, m)
    desc, count, ocount = u8(dev, *lead, m, 128), i32(dev, *lead), i32(dev, *lead, max(O, 0))
    ws = workspace(dev, nws, at_least=16)
    check(lib().skimi_sift_features(ptr(fr), N, H, W, ch, O, M, ptr(box), ptr(_taps_on(dev)), ptr(xy), ptr(xyl), ptr(octv), ptr(lay),
                                    ptr(sig), ptr(resp), ptr(ang), ptr(desc), ptr(count), ptr(ocount), ptr(ws), nws, current_stream()),
          "skimi_sift_features")
    return SiftFeatures(xy, xyl, octv, lay, sig, resp, ang, desc, count, ocount)


def match_l2(d1: torch.Tensor, n1: torch.Tensor, d2: torch.Tensor, n2: torch.Tensor, ratio=0.75, cross_check: bool = False,
             max_distance2=None, max_matches: int = 1000) -> L2Matches:
    """Brute-force L2 matching of descriptor sets d1 [..., M1, 128] (query) and d2 [..., M2, 128] (train), uint8 device tensors
    under common leading axes, of which the first n1 [...] and n2 [...] (device) rows count.  Exact int32 squared distances;
    each query's nearest and second-nearest train descriptor by (distance, index): s1, s2.  ratio = r keeps the query iff
    there are two train rows and (double)s1 < (r r) (double)s2 (None: no ratio test); cross_check keeps it iff the train's
    nearest query is that query; max_distance2 bounds s1.  The kept pairs by (s1, query), the first max_matches of them:
    knnMatch(k = 2) + Lowe's ratio test + sorted(key=distance)[:max_matches] of the reference.  Two launches, nothing is read
    back."""
    lead, B, a, na, b, nb = descriptor_sets("match_l2", d1, n1, d2, n2, 128, torch.uint8, convert=False)
    dev, mm = d1.device, int(max_matches)
    M1, M2 = int(d1.shape[-2]), int(d2.shape[-2])
    m = max(mm, 0)
    pairs, dist2, second2, count = i32(dev, *lead, m, 2), i32(dev, *lead, m), i32(dev, *lead, m), i32(dev, *lead)
    nws = 8 * B * (M1 + M2) + 4 * B * M1
    ws = workspace(dev, nws, at_least=16)
    check(lib().skimi_match_l2(ptr(a), ptr(na), M1, ptr(b), ptr(nb), M2, B, int(bool(cross_check)),
                               -1.0 if ratio is None else float(ratio), -1 if max_distance2 is None else int(max_distance2), mm,
                               ptr(pairs), ptr(dist2), ptr(second2), ptr(count), ptr(ws), nws, current_stream()), "skimi_match_l2")
    return L2Matches(pairs, dist2, second2, count)
