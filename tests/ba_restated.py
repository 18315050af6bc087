"""Float64 torch-autograd restatement of the bundle adjustment (csrc/ba.hip, geometry.bundle_adjust; DESIGN §2 "BA"):
the five losses of bundle_adjustment/loss.py, the w parameterisation of mode full (R = Exp(w) R0) and Adam written out
as the rules state it.  The GPU tests compare the kernel with this; tests/golden/ba_losses.npz pins this against the
reference's own loss functions and torch.optim.Adam."""
from __future__ import annotations

import numpy as np
import torch

BONES = [(11, 13), (13, 15), (12, 14), (14, 16), (5, 7), (7, 9), (6, 8), (8, 10), (5, 6), (11, 12), (5, 11), (6, 12)]
DEFAULT_WEIGHTS = {"ba_weight_reproj": 1.0, "ba_weight_smooth": 1e-2, "ba_weight_baseline": 1e-2,
                   "ba_weight_bone_length": 1e-2, "ba_weight_pose_temporal": 1e-2}
SMALL_ANGLE2 = 1e-8
BETA1, BETA2, EPS = 0.9, 0.999, 1e-8


def weight_list(weights=None):
    w = dict(DEFAULT_WEIGHTS)
    w.update(weights or {})
    return [w[k] for k in DEFAULT_WEIGHTS]


def hat(w):
    z = torch.zeros_like(w[..., 0])
    return torch.stack([torch.stack([z, -w[..., 2], w[..., 1]], -1),
                        torch.stack([w[..., 2], z, -w[..., 0]], -1),
                        torch.stack([-w[..., 1], w[..., 0], z], -1)], -2)


def rodrigues(w):
    """Exp([w]x) = I + A K + B K^2; the Taylor branch below theta^2 = 1e-8 sits behind torch.where, with the large
    branch fed a safe angle there (autograd of sin(th)/th at th = 0 is NaN otherwise)."""
    s = (w * w).sum(-1)[..., None, None]
    small = s < SMALL_ANGLE2
    s_safe = torch.where(small, torch.ones_like(s), s)
    th = torch.sqrt(s_safe)
    A = torch.where(small, 1.0 - s / 6.0 + s * s / 120.0, torch.sin(th) / th)
    B = torch.where(small, 0.5 - s / 24.0 + s * s / 720.0, (1.0 - torch.cos(th)) / s_safe)
    K = hat(w)
    eye = torch.eye(3, dtype=w.dtype, device=w.device).expand(K.shape)
    return eye + A * K + B * (K @ K)


def centres(R, t):
    return -(R.transpose(-1, -2) @ t[..., None])[..., 0]


def terms(X, R, t, K, x2d, conf, weights=None):
    """The five weighted loss terms (loss.py formulas) -> tensor [5]: reprojection, camera smoothness, baseline,
    bone length, pose temporal.  T = 1: both temporal terms are 0."""
    w_rep, w_smooth, w_base, w_bone, w_temp = weight_list(weights)
    T, J = X.shape[0], X.shape[1]
    Xc = (R[:, :, None] @ X[:, None, :, :, None])[..., 0] + t[:, :, None]       # (T,C,J,3)
    Z = Xc[..., 2:3].clamp(min=1e-6)
    xy = Xc[..., 0:2] / Z
    xy1 = torch.cat([xy, torch.ones_like(Z)], -1)
    proj = (K[None, :, None] @ xy1[..., None])[..., 0][..., :2]
    diff = ((proj - x2d) ** 2).sum(-1)
    rep = w_rep * (conf * diff).sum() / (conf.sum() + 1e-6)
    Cc = centres(R, t)
    zero = X.new_zeros(())
    smooth = w_smooth * ((Cc[1:] - Cc[:-1]) ** 2).mean() if T > 1 else zero
    if Cc.shape[1] >= 2:
        b = torch.norm(Cc[:, 0] - Cc[:, 1], dim=-1)
        base = w_base * ((b - b.mean().detach()) ** 2).mean()
    else:
        base = zero
    lens = [torch.norm(X[:, i] - X[:, j], dim=-1) for i, j in BONES if i < J and j < J]
    if lens:
        L = torch.stack(lens, -1)
        bone = w_bone * ((L - L.mean(0, keepdim=True).detach()) ** 2).mean()
    else:
        bone = zero
    temp = w_temp * ((X[1:] - X[:-1]) ** 2).mean() if T > 1 else zero
    return torch.stack([rep, smooth, base, bone, temp])


def _t(a, device):
    a = a.detach() if isinstance(a, torch.Tensor) else torch.tensor(np.asarray(a))
    return a.to(device, torch.float64).clone()


def run(K, R0, t0, X0, x2d, conf, mode="pose_only", num_iters=200, lr=1e-3, weights=None, device="cpu"):
    """Adam on the loss: p <- p - (lr / (1 - b1^k)) m / (sqrt(v) / sqrt(1 - b2^k) + eps), k from 1.
    -> (R, t, X, history [num_iters, 6]) as float64 tensors on `device`; history row i at the iterate before step i+1."""
    K, R0, t0, X0, x2d, conf = (_t(a, device) for a in (K, R0, t0, X0, x2d, conf))
    X = X0.clone().requires_grad_(True)
    t = t0.clone().requires_grad_(mode != "pose_only")
    w = torch.zeros_like(t0).requires_grad_(mode == "full")
    params = [X] + ([t] if mode != "pose_only" else []) + ([w] if mode == "full" else [])
    m = [torch.zeros_like(p) for p in params]
    v = [torch.zeros_like(p) for p in params]
    hist = torch.zeros((num_iters, 6), dtype=torch.float64, device=device)
    for k in range(1, num_iters + 1):
        R = rodrigues(w) @ R0 if mode == "full" else R0
        tm = terms(X, R, t, K, x2d, conf, weights)
        loss = tm[0] + tm[1] + tm[2] + tm[3] + tm[4]
        hist[k - 1, 0] = loss.detach()
        hist[k - 1, 1:] = tm.detach()
        grads = torch.autograd.grad(loss, params)
        with torch.no_grad():
            bc1 = 1.0 - BETA1 ** k
            bc2_sqrt = (1.0 - BETA2 ** k) ** 0.5
            for p, g, mm, vv in zip(params, grads, m, v):
                mm.copy_(BETA1 * mm + (1.0 - BETA1) * g)
                vv.copy_(BETA2 * vv + (1.0 - BETA2) * (g * g))
                p.sub_((lr / bc1) * (mm / (vv.sqrt() / bc2_sqrt + EPS)))
    with torch.no_grad():
        R = rodrigues(w) @ R0 if mode == "full" else R0.clone()
    return R, t.detach().clone(), X.detach().clone(), hist
