"""Bundle adjustment of a clip's cameras and joints (csrc/ba.hip; C-ABI: skimi_ba_workspace_bytes, skimi_bundle_adjust):
run_local_ba of vggt/multi_view_process.py:523-564 with the losses of bundle_adjustment/loss.py.

Rules (DESIGN §2 "BA"): float64 throughout; mode full optimises w [T,C,3] with R = Exp(w) R0 (Rodrigues, Taylor
branch below theta^2 = 1e-8); the baseline and bone-length means are taken at the current iterate and held
constant; a clamped Z (< 1e-6) and a zero-length bone or baseline pass no gradient; the two temporal terms are 0 at
T = 1; Adam with torch's defaults.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import torch

from .._args import f64, shapes, upload_f64, workspace
from .._lib import check, current_stream, lib, ptr

BA_MODES = {"pose_only": 0, "pose_cam_t": 1, "full": 2}
# cfg.bundle_adjustment key -> default weight of its loss in bundle_adjustment/loss.py, in the order of the C-ABI
BA_WEIGHT_KEYS = {"ba_weight_reproj": 1.0, "ba_weight_smooth": 1e-2, "ba_weight_baseline": 1e-2,
                  "ba_weight_bone_length": 1e-2, "ba_weight_pose_temporal": 1e-2}
BA_PLACEMENTS = {"auto": 0, "lds": 1, "workspace": 2}


@dataclass
class BAResult:
    mode: str
    R: torch.Tensor          # float64 [T, C, 3, 3]
    t: torch.Tensor          # float64 [T, C, 3]
    X: torch.Tensor          # float64 [T, J, 3]
    history: torch.Tensor    # float64 [num_iters, 6]: total, reprojection, smoothness, baseline, bone length, temporal


def ba_weights(weights=None) -> list:
    """The five loss weights in C-ABI order from a mapping keyed like cfg.bundle_adjustment (absent keys take the
    default `w` of their loss.py function)."""
    weights = dict(weights or {})
    unknown = sorted(set(weights) - set(BA_WEIGHT_KEYS))
    if unknown:
        raise ValueError(f"unknown bundle-adjustment weight keys {unknown}; known: {list(BA_WEIGHT_KEYS)}")
    return [float(weights.get(k, d)) for k, d in BA_WEIGHT_KEYS.items()]


def bundle_adjust(K, R, t, X, x2d, conf, modes=("pose_only",), num_iters: int = 200, lr: float = 1e-3, weights=None,
                  placement: str = "auto") -> list:
    """Bundle adjustment of one clip, every mode in ONE launch (one workgroup per mode): K [C,3,3], R [T,C,3,3],
    t [T,C,3] (world -> camera), X [T,J,3], x2d [T,C,J,2] pixels, conf [T,C,J]; host arrays or device tensors.
    `modes`: a mode name or a sequence of them (pose_only: X; pose_cam_t: X, t; full: X, t, R).  `weights`: a mapping
    with cfg.bundle_adjustment's ba_weight_* keys.  `placement` ("auto", "lds", "workspace"): where the state lives;
    it does not change the results.  -> [BAResult] in the order of `modes`, float64 device tensors."""
    if isinstance(modes, str):
        modes = (modes,)
    modes = list(modes)
    bad = [m for m in modes if m not in BA_MODES]
    if bad or not modes:
        raise ValueError(f"unknown bundle-adjustment modes {bad or modes}; known: {list(BA_MODES)}")
    if placement not in BA_PLACEMENTS:
        raise ValueError(f"unknown placement {placement!r}; known: {list(BA_PLACEMENTS)}")
    w = ba_weights(weights)
    dev = next((a.device for a in (K, R, t, X, x2d, conf) if isinstance(a, torch.Tensor) and a.is_cuda),
               torch.device("cuda", torch.cuda.current_device()))
    K, R, t, X, x2d, conf = (upload_f64(a, dev) for a in (K, R, t, X, x2d, conf))
    if X.dim() != 3 or X.shape[-1] != 3:
        raise ValueError(f"bundle_adjust: X must be [T, J, 3], got {tuple(X.shape)}")
    T, J = X.shape[0], X.shape[1]
    Cn = K.shape[0] if K.dim() == 3 else -1
    shapes("bundle_adjust", (("K", K, (Cn, 3, 3)), ("R", R, (T, Cn, 3, 3)), ("t", t, (T, Cn, 3)), ("x2d", x2d, (T, Cn, J, 2)),
                             ("conf", conf, (T, Cn, J))))
    P = len(modes)
    R_out, t_out, X_out = f64(dev, P, T, Cn, 3, 3), f64(dev, P, T, Cn, 3), f64(dev, P, T, J, 3)
    hist = f64(dev, P, int(num_iters), 6)
    ws = workspace(dev, lib().skimi_ba_workspace_bytes(T, Cn, J, P))
    codes = (C.c_int32 * P)(*[BA_MODES[m] for m in modes])
    check(lib().skimi_bundle_adjust(ptr(K), ptr(R), ptr(t), ptr(X), ptr(x2d), ptr(conf), T, Cn, J, codes, P, int(num_iters),
                                    float(lr), *w, BA_PLACEMENTS[placement], ptr(R_out), ptr(t_out), ptr(X_out),
                                    ptr(hist) if hist.numel() else None, ptr(ws), ws.numel(), current_stream()),
          "skimi_bundle_adjust")
    return [BAResult(m, R_out[p], t_out[p], X_out[p], hist[p]) for p, m in enumerate(modes)]
