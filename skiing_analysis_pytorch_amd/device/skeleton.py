"""Conversion between the COCO-17 and the H36M-17 skeleton on the device (csrc/skeleton.hip; C-ABI: skimi_convert_skeleton):
VideoPose3D/coco_hm36.py; the host form is the package's skeleton.py; rules: DESIGN §2 "Skeleton conversion".
"""
from __future__ import annotations

import numpy as np
import torch

from .._args import f64
from .._lib import SkimiError, check, current_stream, lib, ptr

SKELETON_DIRECTIONS = {"coco_to_h36m": 0, "h36m_to_coco": 1}


def convert_skeleton(X, direction: str, synthesize_head: bool = True, synthesize_face: bool = False) -> torch.Tensor:
    """skeleton.coco_to_h36m / skeleton.h36m_to_coco in one launch: X (17, C) or (T, 17, C), C = 2 or 3, a device tensor or a
    host array (uploaded to the current device) -> float64 device tensor of the same shape.  synthesize_head belongs to
    "coco_to_h36m", synthesize_face to "h36m_to_coco" (the reference's clip-mean shoulder test is kept)."""
    if direction not in SKELETON_DIRECTIONS:
        raise ValueError(f"convert_skeleton: direction must be one of {sorted(SKELETON_DIRECTIONS)}")
    if isinstance(X, torch.Tensor):
        if not X.is_cuda:
            raise SkimiError("convert_skeleton needs a device tensor or a host array")
        X = X.to(torch.float64).contiguous()
    else:
        X = torch.as_tensor(np.ascontiguousarray(np.asarray(X, dtype=np.float64))).to(torch.device("cuda", torch.cuda.current_device()))
    if X.dim() not in (2, 3) or X.shape[-2] != 17 or X.shape[-1] not in (2, 3):
        raise ValueError(f"convert_skeleton: need (17, C) or (T, 17, C) with C in (2, 3), got {list(X.shape)}")
    T = X.shape[0] if X.dim() == 3 else 1
    Y = f64(X.device, *X.shape)
    syn = synthesize_head if direction == "coco_to_h36m" else synthesize_face
    check(lib().skimi_convert_skeleton(ptr(X), T, int(X.shape[-1]), SKELETON_DIRECTIONS[direction], int(bool(syn)), ptr(Y),
                                       current_stream()), "skimi_convert_skeleton")
    return Y
