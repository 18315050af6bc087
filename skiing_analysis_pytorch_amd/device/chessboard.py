"""Chessboard corners from whole frames (csrc/chessboard.hip; C-ABI: skimi_chess_workspace_bytes, skimi_chess_candidates,
skimi_corner_subpix): camera_calibration/main.py:80-90 (find_chessboard_corners = cv2.findChessboardCorners +
cv2.cornerSubPix) under the project's own rules; the reference's names are the package's calibration.py, which also orders
the candidates into a board on the host; rules: include/skimi.h, DESIGN §2 "Chessboard corners".

Frames are uint8 [F, H, W, ch] or [C, F, H, W, ch] device tensors, ch 1, 3 or 4 with colour channels in cv2's B, G, R order
(preprocess.undistort_images' convention); every result carries the frames' leading axes.
"""
from __future__ import annotations

from typing import NamedTuple

import torch

from .._args import frame_clip, i32, on_device, to_dev, u8, workspace
from .._lib import check, current_stream, lib, ptr

CHESS_MAX_NMS, SUBPIX_MAX_WIN, SUBPIX_MAX_ITERS = 15, 15, 1000


class ChessCandidates(NamedTuple):
    """chessboard_candidates' outputs (int32 device tensors; M = max_candidates)."""
    xy: torch.Tensor         # [..., M, 2]: (x, y) in ascending pixel order, (-1, -1) behind the last candidate
    response: torch.Tensor   # [..., M]: the ChESS response R there, 0 behind the last candidate
    count: torch.Tensor      # [...]: the frame's candidates, uncapped (count > M: the rows hold the first M)
    rmax: torch.Tensor       # [...]: the frame's largest response


class SubpixResult(NamedTuple):
    """corner_subpix's outputs (device tensors)."""
    points: torch.Tensor     # float64 [..., M, 2]: the refined points; the start where ok is False
    ok: torch.Tensor         # bool [..., M]: refined and ended within the half window of its start


def chessboard_candidates(frames: torch.Tensor, threshold: int = 38, nms_radius: int = 4,
                          max_candidates: int = 1024) -> ChessCandidates:
    """Chessboard corner candidates of every frame in three launches: gray, a 3 x 3 binomial blur, the ChESS response on the
    radius-5 ring and the frame's maximum; then the pixels with R > 0 and 256 R > threshold rmax that are the maximum of their
    (2 nms_radius + 1)^2 window (ties to the earlier pixel), compacted in pixel order.  All integer: bitwise reproducible, and
    a frame gives the same bits alone and in a batch.  Nothing is read back."""
    fr, five = frame_clip("chessboard_candidates", frames)
    C, F, H, W, ch = (int(s) for s in fr.shape)
    N, M, dev = C * F, int(max_candidates), fr.device
    if N < 1 or M < 1:
        raise ValueError(f"chessboard_candidates: need at least one frame and max_candidates >= 1, got {N} frames, {M}")
    lead = (C, F) if five else (F,)
    xy, resp, count, rmax = i32(dev, *lead, M, 2), i32(dev, *lead, M), i32(dev, *lead), i32(dev, *lead)
    nws = int(lib().skimi_chess_workspace_bytes(N, H, W))
    ws = workspace(dev, nws, at_least=8)
    check(lib().skimi_chess_candidates(ptr(fr), N, H, W, ch, int(threshold), int(nms_radius), M, ptr(xy), ptr(resp), ptr(count),
                                       ptr(rmax), ptr(ws), nws, current_stream()), "skimi_chess_candidates")
    return ChessCandidates(xy, resp, count, rmax)


def corner_subpix(frames: torch.Tensor, points: torch.Tensor, count=None, win=(5, 5), iters: int = 30) -> SubpixResult:
    """cv2.cornerSubPix's iteration in float64 on any points of the frames, in one launch: points [..., M, 2] (device; x, y in
    pixels, any real dtype) under the frames' leading axes, count [...] int (device) or None: only the first count points of
    a frame are refined; win = the half window (wx, wy), 1 .. 15 each (cv2's winSize).  Exactly `iters` rounds, no epsilon
    stop.  A point that ends more than the half window from its start, starts outside the frame or is not finite goes back
    to its start with ok False."""
    fr, five = frame_clip("corner_subpix", frames)
    on_device("corner_subpix", points=points, count=count)
    C, F, H, W, ch = (int(s) for s in fr.shape)
    lead = (C, F) if five else (F,)
    if points.dim() != len(lead) + 2 or tuple(points.shape[:len(lead)]) != lead or points.shape[-1] != 2:
        raise ValueError(f"corner_subpix: points must be {list(lead)} + [M, 2], got {list(points.shape)}")
    if count is not None and tuple(count.shape) != lead:
        raise ValueError(f"corner_subpix: count must be {list(lead)}, got {list(count.shape)}")
    wx, wy = (int(w) for w in win)
    dev, M = fr.device, int(points.shape[-2])
    pts, cnt = to_dev(points, dev=dev), to_dev(count, torch.int32, dev)
    out, ok = torch.empty_like(pts), u8(dev, *lead, M)
    if pts.numel() == 0:
        return SubpixResult(out, ok.bool())
    check(lib().skimi_corner_subpix(ptr(fr), C * F, H, W, ch, ptr(pts), ptr(cnt), M, wx, wy, int(iters), ptr(out), ptr(ok),
                                    current_stream()), "skimi_corner_subpix")
    return SubpixResult(out, ok.bool())
