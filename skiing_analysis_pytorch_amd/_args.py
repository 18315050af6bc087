"""The argument idioms of the wrappers under device/ (and of preprocess.py, bev.py), once each: device checks, conversions,
shape tables, output and workspace allocation, the leading-axis rule, and the small host arrays that travel by value.

A wrapper reads top to bottom as checks, allocations, one check(lib().skimi_...(...)) and the result tuple.  Nothing here
synchronises, reads a tensor back or copies a tensor that already conforms (`.to` and `.contiguous` return their input
then).  `fn` is the calling function's name: every message starts with it.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from ._lib import SkimiError


# ---- device checks and conversions ---------------------------------------------------------------------------------------
def on_device(fn, *tensors, what="device tensors", **named):
    """Every argument is a device tensor (None: an optional argument that is absent), else SkimiError.  Arguments passed by
    keyword are named in the message with the device they are on."""
    for a in tensors:
        if a is not None and not (isinstance(a, torch.Tensor) and a.is_cuda):
            raise SkimiError(f"{fn} needs {what}")
    for name, a in named.items():
        if a is not None and not (isinstance(a, torch.Tensor) and a.is_cuda):
            raise SkimiError(f"{fn} needs {what} ({name} is on {getattr(a, 'device', 'the host')})")


def to_dev(a, dtype=torch.float64, dev=None):
    """-> contiguous `dtype` on dev (default: where it is); None stays None"""
    return None if a is None else a.to(a.device if dev is None else dev, dtype).contiguous()


def upload_f64(a, dev):
    """a tensor, or a host array (made float64 on the host) -> contiguous float64 on dev"""
    return to_dev(a if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a, dtype=np.float64)), dev=dev)


def contig_as(a, dtype=torch.float32):
    """-> contiguous first, then `dtype` (the float32 wrappers' order); None stays None"""
    return None if a is None else a.contiguous().to(dtype)


def device_tensor(fn, a):
    """a itself, checked by on_device"""
    on_device(fn, a)
    return a


def f64_dev(fn, a, dev=None):
    """device_tensor + to_dev in float64"""
    return to_dev(device_tensor(fn, a), dev=dev)


def host_f64(a) -> np.ndarray:
    """a small host array (NumPy, list, CPU tensor; a device tensor is copied back) -> contiguous float64"""
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64))


def host_ptr(a):
    """the address of a host array for a by-value argument (None passes NULL)"""
    return None if a is None else a.ctypes.data


# ---- shapes ----------------------------------------------------------------------------------------------------------
def shapes(fn, rows, f32_on=None):
    """rows of (argument name, tensor or None, wanted shape): ValueError with the wanted and the received shape.  f32_on=dev
    is the strictness of the launch fast paths, which must not convert: every tensor must already be contiguous float32
    on dev (SkimiError for the device, checked row by row ahead of the row's shape)."""
    for name, a, want in rows:
        if a is None:
            continue
        if f32_on is None:
            if tuple(a.shape) != tuple(want):
                raise ValueError(f"{fn}: {name} must be {list(want)}, got {list(a.shape)}")
            continue
        if not a.is_cuda or a.device != f32_on:
            raise SkimiError(f"{fn} needs device tensors on one device ({name} is on {a.device})")
        if tuple(a.shape) != tuple(want) or a.dtype != torch.float32 or not a.is_contiguous():
            raise ValueError(f"{fn}: {name} must be contiguous float32 {list(want)}, got {a.dtype} {list(a.shape)}")


def add_lead(a, ndim):
    """The leading-axis rule: an input one axis short of `ndim` is one clip / one group -> (a with the axis, whether it was
    added).  strip_lead takes it off the results again."""
    single = a.dim() == ndim - 1
    return (a[None] if single else a), single


def strip_lead(results, single):
    return tuple(a[0] for a in results) if single else tuple(results)


def clips(fn, X, dev=None):
    """[B, T, J, 3] float64 device clips; a [T, J, 3] input is one clip"""
    X, _ = add_lead(f64_dev(fn, X, dev), 4)
    if X.dim() != 4 or X.shape[3] != 3:
        raise ValueError(f"{fn}: need [B, T, J, 3] or [T, J, 3], got {list(X.shape)}")
    return X


def lengths(fn, lens, B, dev):
    """None, or the clips' lengths [B] (host integers or a tensor) -> int32 on dev"""
    if lens is None:
        return None
    len_t = lens if isinstance(lens, torch.Tensor) else torch.as_tensor(np.asarray(lens, dtype=np.int64))
    if tuple(len_t.shape) != (B,):
        raise ValueError(f"{fn}: lengths must be [{B}], got {list(len_t.shape)}")
    return len_t.to(dev, torch.int32).contiguous()


def index_list(fn, what, pairs, limit):
    """a list of index pairs -> (int32 C array of the flattened pairs, their number); values are clipped to int32"""
    a = np.asarray(list(pairs), dtype=np.int64).reshape(-1, 2) if len(pairs) else np.zeros((0, 2), dtype=np.int64)
    if a.shape[0] > limit:
        raise ValueError(f"{fn}: {a.shape[0]} {what}, at most {limit}")
    flat = [int(np.clip(v, -2 ** 31, 2 ** 31 - 1)) for v in a.reshape(-1)]
    return (C.c_int32 * max(len(flat), 1))(*flat), a.shape[0]


def group_split(N, group_size):
    """-> (group size, number of whole groups) of N consecutive points; None: one group.  A size that does not divide N is
    the library's to refuse."""
    gs = N if group_size is None else int(group_size)
    return gs, (N // gs if gs >= 1 and N >= 1 else 0)


# ---- allocation ------------------------------------------------------------------------------------------------------
def f64(dev, *shape):
    return torch.empty(shape, dtype=torch.float64, device=dev)


def f32(dev, *shape):
    return torch.empty(shape, dtype=torch.float32, device=dev)


def i32(dev, *shape):
    return torch.empty(shape, dtype=torch.int32, device=dev)


def u8(dev, *shape):
    return torch.empty(shape, dtype=torch.uint8, device=dev)


def workspace(dev, nbytes, at_least=0, optional=False, as_f64=False):
    """`nbytes` of scratch on dev.  The conventions the C side checks `ws` against: optional=True passes NULL for a
    zero-byte request; at_least=8 keeps the pointer non-NULL; as_f64=True allocates float64 elements."""
    nbytes = int(nbytes)
    if optional and not nbytes:
        return None
    n = max(nbytes, at_least)
    return f64(dev, n // 8) if as_f64 else u8(dev, n)


# ---- host arrays that travel by value --------------------------------------------------------------------------------
def camera_matrices(fn, what, M, C):
    """[3, 3] or [C, 3, 3] host matrix -> float64 [C or 1, 3, 3]; only fx, fy, cx, cy are part of the model"""
    M = host_f64(M)
    if M.shape[-2:] != (3, 3) or M.ndim not in (2, 3):
        raise ValueError(f"{fn}: {what} must be [3, 3] or [C, 3, 3], got {list(M.shape)}")
    M = M.reshape(-1, 3, 3)
    if C is not None and M.shape[0] != C:
        if M.shape[0] != 1:
            raise ValueError(f"{fn}: {what} holds {M.shape[0]} cameras, K holds {C}")
        M = np.ascontiguousarray(np.broadcast_to(M, (C, 3, 3)))
    if not (np.isfinite(M[:, [0, 1, 0, 1], [0, 1, 2, 2]]).all() and (M[:, 0, 0] != 0).all() and (M[:, 1, 1] != 0).all()):
        raise ValueError(f"{fn}: {what} needs finite, non-zero focal lengths and a finite principal point")
    return M


def per_camera_coeffs(fn, d, C):
    """lens coefficients [12] or [1 or C, 12] (lens_coeffs' result) -> contiguous [C, 12], one row per camera"""
    if d.ndim > 2 or (d.ndim == 2 and d.shape[0] not in (1, C)):
        raise ValueError(f"{fn}: dist must be [k] or [{C}, k], got {list(d.shape)}")
    return np.ascontiguousarray(np.broadcast_to(d.reshape(-1, 12), (C, 12)))


# ---- uint8 frame clips (preprocess.undistort_images, preprocess.warp_perspective) ------------------------------------
def frame_clip(fn, frames):
    """uint8 [F, H, W, ch] or [C, F, H, W, ch] device frames -> (contiguous [C, F, H, W, ch], whether five axes came in)"""
    if not isinstance(frames, torch.Tensor) or not frames.is_cuda or frames.dtype != torch.uint8 or frames.dim() not in (4, 5):
        raise SkimiError(f"{fn} needs a uint8 [F, H, W, ch] or [C, F, H, W, ch] device tensor")
    five = frames.dim() == 5
    fr = frames.contiguous() if five else frames.contiguous()[None]
    if fr.shape[4] not in (1, 3, 4):
        raise ValueError(f"{fn}: 1, 3 or 4 channels, got {int(fr.shape[4])}")
    return fr, five


def frame_out(fn, fr, five, ow, oh, out):
    """the result of a frame clip fr at (ow, oh): `out` checked, or a new tensor"""
    C, F, H, W, ch = (int(s) for s in fr.shape)
    if ow < 1 or oh < 1 or H < 1 or W < 1:
        raise ValueError(f"{fn}: empty frame ({W} x {H} -> {ow} x {oh})")
    shape = (C, F, oh, ow, ch) if five else (F, oh, ow, ch)
    if out is None:
        return u8(fr.device, *shape)
    if not out.is_cuda or out.device != fr.device or out.dtype != torch.uint8 or tuple(out.shape) != shape or not out.is_contiguous():
        raise ValueError(f"{fn}: out must be a contiguous uint8 device tensor {list(shape)}")
    return out


# ---- image features and their matchers (device/features.py, device/sift.py) ------------------------------------------
def feature_frames(fn, frames, roi):
    """The frames and boxes of a feature extractor (device/features.py, device/sift.py) -> (frame_clip's [C, F, H, W, ch], the
    number of frames, their leading axes, roi [..., 4] under those axes as float64 on the frames' device or None)"""
    fr, five = frame_clip(fn, frames)
    on_device(fn, roi=roi)
    C, F = int(fr.shape[0]), int(fr.shape[1])
    if C * F < 1:
        raise ValueError(f"{fn}: need at least one frame, got {C * F}")
    lead = (C, F) if five else (F,)
    if roi is not None and tuple(roi.shape) != (*lead, 4):
        raise ValueError(f"{fn}: roi must be {list(lead)} + [4], got {list(roi.shape)}")
    return fr, C * F, lead, to_dev(roi, dev=fr.device)


def descriptor_sets(fn, d1, n1, d2, n2, width, dtype, convert):
    """The sets of a brute-force matcher: d1 [..., M1, width], d2 [..., M2, width] under common leading axes, n1, n2 [...]
    -> (the leading axes, the number of pairs of sets, d1, n1, d2, n2 contiguous on d1's device, descriptors as `dtype`
    and counts as int32).  convert=False: descriptors of another dtype are refused."""
    on_device(fn, d1=d1, n1=n1, d2=d2, n2=n2)
    lead = tuple(d1.shape[:-2])
    if d1.dim() < 2 or d1.shape[-1] != width or d2.dim() != d1.dim() or d2.shape[-1] != width or tuple(d2.shape[:-2]) != lead:
        raise ValueError(f"{fn}: need d1 [..., M1, {width}] and d2 [..., M2, {width}] under common leading axes, got {list(d1.shape)}, "
                         f"{list(d2.shape)}")
    if not convert and (d1.dtype != dtype or d2.dtype != dtype):
        raise ValueError(f"{fn}: descriptors must be {str(dtype).replace('torch.', '')}, got {d1.dtype}, {d2.dtype}")
    if tuple(n1.shape) != lead or tuple(n2.shape) != lead:
        raise ValueError(f"{fn}: n1 and n2 must be {list(lead)}, got {list(n1.shape)}, {list(n2.shape)}")
    B = int(np.prod(lead, dtype=np.int64))
    if B < 1:
        raise ValueError(f"{fn}: need at least one pair of sets, got leading axes {list(lead)}")
    dev = d1.device
    return lead, B, to_dev(d1, dtype, dev), to_dev(n1, torch.int32, dev), to_dev(d2, dtype, dev), to_dev(n2, torch.int32, dev)



# ---- masks (device/masks.py) -----------------------------------------------------------------------------------------
MASK_MAX_SIDE = 4096


def mask_batch(fn, masks, ndim=3, name="masks"):
    """bool or uint8 device masks [..., H, W] with `ndim` axes, or one axis fewer (add_lead's rule) -> (contiguous uint8 of
    `ndim` axes, whether the axis was added).  Everything that is wrong is a ValueError, a host tensor included; the leading
    axes may be empty, the sides may not."""
    if not isinstance(masks, torch.Tensor) or not masks.is_cuda:
        raise ValueError(f"{fn}: {name} must be a device tensor (it is on {getattr(masks, 'device', 'the host')})")
    if masks.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f"{fn}: {name} must be bool or uint8, got {masks.dtype}")
    if masks.dim() not in (ndim - 1, ndim):
        raise ValueError(f"{fn}: {name} must have {ndim - 1} or {ndim} axes [..., H, W], got {list(masks.shape)}")
    m, single = add_lead(masks.contiguous(), ndim)
    H, W = int(m.shape[-2]), int(m.shape[-1])
    if not (1 <= H <= MASK_MAX_SIDE and 1 <= W <= MASK_MAX_SIDE):
        raise ValueError(f"{fn}: {name} of {W} x {H} pixels, sides must be 1 .. {MASK_MAX_SIDE}")
    if m.numel() >= 2 ** 31:
        raise ValueError(f"{fn}: {name} holds {m.numel()} pixels, at most 2^31 - 1")
    return (m.view(torch.uint8) if m.dtype == torch.bool else m), single


def i64(dev, *shape):
    return torch.empty(shape, dtype=torch.int64, device=dev)
