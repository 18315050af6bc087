"""Float64 restatement of the reference's TemporalModel(dense=True) forward (VideoPose3D/common/model.py:79-138) and of
the inference slice of run_video_pose_3d around it (run.py:191-199 normalisation, :1070-1081 UnchunkedGenerator
padding + flip TTA, :979-986 un-flip + mean).  torch.nn.functional.conv1d in float64, BatchNorm in eval mode
(eps 1e-5), dropout the identity.

The rules of the dense model, as DESIGN §2 (a20) pins them:
- block i >= 1 keeps the dilated model's pad_i = (fw_i - 1) * fw_0 * ... * fw_{i-1} / 2 and causal shift, so the
  receptive field and every layer's output length are those of the dilated model;
- its first conv has 2 * pad_i + 1 taps at dilation 1, no bias, then BN and ReLU; then a 1x1 conv, BN, ReLU and the
  residual x[:, :, pad + shift : L - pad + shift];
- expand_conv, the 1x1 convs and shrink are the dilated model's.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

KPS_LEFT = [1, 3, 5, 7, 9, 11, 13, 15]
KPS_RIGHT = [2, 4, 6, 8, 10, 12, 14, 16]
JOINTS_LEFT = [4, 5, 6, 11, 12, 13]
JOINTS_RIGHT = [1, 2, 3, 14, 15, 16]


def pads(filter_widths, causal):
    """(pad, causal_shift) per layer, model.py:31,105-110"""
    pad, shift = [filter_widths[0] // 2], [filter_widths[0] // 2 if causal else 0]
    nd = filter_widths[0]
    for fw in filter_widths[1:]:
        pad.append((fw - 1) * nd // 2)
        shift.append(fw // 2 * nd if causal else 0)
        nd *= fw
    return pad, shift


def receptive_field(filter_widths):
    return 1 + 2 * sum(pads(filter_widths, False)[0])


def _bn(x, sd, prefix):
    g = sd[prefix + ".weight"].double()
    b = sd[prefix + ".bias"].double()
    mu = sd[prefix + ".running_mean"].double()
    var = sd[prefix + ".running_var"].double()
    return (x - mu[None, :, None]) / torch.sqrt(var[None, :, None] + 1e-5) * g[None, :, None] + b[None, :, None]


def forward(sd, x, filter_widths, causal=False):
    """x [B, L, J, 2] -> [B, L - rf + 1, J_out, 3] (float64)"""
    x = torch.as_tensor(x).double()
    B, L = x.shape[:2]
    h = x.reshape(B, L, -1).permute(0, 2, 1)
    h = torch.relu(_bn(F.conv1d(h, sd["expand_conv.weight"].double()), sd, "expand_bn"))
    pad, shift = pads(filter_widths, causal)
    for i in range(1, len(filter_widths)):
        res = h[:, :, pad[i] + shift[i]: h.shape[2] - pad[i] + shift[i]]
        w = sd[f"layers_conv.{2 * (i - 1)}.weight"].double()
        assert w.shape[2] == 2 * pad[i] + 1, (w.shape, pad[i])
        h = torch.relu(_bn(F.conv1d(h, w), sd, f"layers_bn.{2 * (i - 1)}"))
        h = res + torch.relu(_bn(F.conv1d(h, sd[f"layers_conv.{2 * (i - 1) + 1}.weight"].double()), sd,
                                 f"layers_bn.{2 * (i - 1) + 1}"))
    h = F.conv1d(h, sd["shrink.weight"].double(), sd["shrink.bias"].double())
    return h.permute(0, 2, 1).reshape(B, -1, sd["shrink.bias"].shape[0] // 3, 3)


def lift_clip(sd, keypoints_px, w, h, filter_widths, causal=False, augment=True):
    """[T, 17, 2] pixel keypoints -> [T, 17, 3] (float64)"""
    kps = np.asarray(keypoints_px, dtype=np.float64)[..., :2] / w * 2 - [1, h / w]
    pad = (receptive_field(filter_widths) - 1) // 2
    shift = pad if causal else 0
    batch = np.pad(kps, ((pad + shift, pad - shift), (0, 0), (0, 0)), "edge")[None]
    if augment:
        batch = np.concatenate((batch, batch), axis=0)
        batch[1, :, :, 0] *= -1
        batch[1, :, KPS_LEFT + KPS_RIGHT] = batch[1, :, KPS_RIGHT + KPS_LEFT]
    pred = forward(sd, torch.from_numpy(batch.astype(np.float32)), filter_widths, causal)
    if augment:
        pred = pred.clone()
        pred[1, :, :, 0] *= -1
        pred[1, :, JOINTS_LEFT + JOINTS_RIGHT] = pred[1, :, JOINTS_RIGHT + JOINTS_LEFT]
        pred = pred.mean(dim=0, keepdim=True)
    return pred[0].numpy()
