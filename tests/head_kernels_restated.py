"""NumPy / torch float64 restatement of the VGGT head and track-head helper kernels (include/skimi.h, "VGGT head and
track-head helper kernels"; csrc/vggt_kernels.hip, csrc/track_kernels.hip).  One plain function per kernel, no cleverness:
this is what the kernels are tested against.  Where an operation is DEFINED by float32 steps (the resize's index
arithmetic, the track input's flow and angle) those steps are single correctly rounded NumPy float32 operations -- the
library is built without contraction or fast-math, so they are bit-reproducible -- and everything else is float64.
Functions that the GPU tests bound return the value and the magnitude `mag` their forward error bound is built from:
the same formula evaluated on absolute values."""
import math

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24            # fp32's unit roundoff, the unit every bound is counted in: one rounding is at most U relative
F32_TINY = 2.0 ** -126    # below the normal range an fp32 result may be flushed: absolute floor of the exp bounds
f32 = np.float32


# ---- 16-bit formats ----
def decode16(bits, f16):
    """uint16 patterns -> float64 values of bf16 (f16 False) or IEEE fp16 (f16 True)"""
    b = np.ascontiguousarray(bits, dtype=np.uint16)
    if f16:
        return b.view(np.float16).astype(np.float64)
    return (b.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def bf16_rne_bits(x):
    """float32 values -> bf16 patterns, round to nearest even (finite values)"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def half_ulp16(v, f16):
    """half a unit in the last place of the 16-bit format at the value v: 2^(e - 8) for bf16 (8 significant bits) and
    2^(max(e, -14) - 11) for fp16 (11 bits, subnormal below 2^-14) with e = floor(log2 |v|) -- between 2^-9 |v| and
    2^-8 |v|, resp. 2^-12 |v| and 2^-11 |v|, in the normal range"""
    e = np.frexp(np.abs(np.asarray(v, np.float64)))[1] - 1
    return np.exp2(np.maximum(e, -14) - 11.0) if f16 else np.exp2(np.maximum(e, -126) - 8.0)


# ---- bilinear resize, align_corners=True ----
def resize_indices(n_in, n_out):
    """ATen's float32 index arithmetic along one axis -> i0, i1 (int64), l0, l1 (float32 values held in float64)"""
    scale = f32(n_in - 1) / f32(n_out - 1) if n_out > 1 else f32(0)
    src = scale * np.arange(n_out, dtype=np.float32)
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    l1 = np.clip(src - i0.astype(np.float32), f32(0), f32(1))
    l0 = f32(1) - l1
    assert src.dtype == l1.dtype == l0.dtype == np.float32
    return i0, i1, l0.astype(np.float64), l1.astype(np.float64)


def uv_add(H, W, tabx, taby):
    """[H, W, C]: c < C/2 ? tabx[X][c] : taby[Y][c - C/2]"""
    tabx, taby = np.asarray(tabx, np.float64), np.asarray(taby, np.float64)
    half = tabx.shape[1]
    return np.concatenate([np.broadcast_to(tabx[None, :, :], (H, W, half)),
                           np.broadcast_to(taby[:, None, :], (H, W, half))], axis=-1)


def resize(x, H, W, tabx=None, taby=None):
    """x [N, h, w, C] -> (v, mag) [N, H, W, C]: v = l0y (l0x p00 + l1x p01) + l1y (l0x p10 + l1x p11) (+ uv) in float64"""
    x = np.asarray(x, np.float64)
    _, h, w, _ = x.shape
    y0, y1, ly0, ly1 = resize_indices(h, H)
    x0, x1, lx0, lx1 = resize_indices(w, W)
    ly0, ly1 = ly0[None, :, None, None], ly1[None, :, None, None]
    lx0, lx1 = lx0[None, None, :, None], lx1[None, None, :, None]

    def lerp(a):
        top, bot = a[:, y0], a[:, y1]
        return ly0 * (lx0 * top[:, :, x0] + lx1 * top[:, :, x1]) + ly1 * (lx0 * bot[:, :, x0] + lx1 * bot[:, :, x1])

    v, mag = lerp(x), lerp(np.abs(x))
    if tabx is not None:
        uv = uv_add(H, W, tabx, taby)[None]
        v, mag = v + uv, mag + np.abs(uv)
    return v, mag


def layernorm(v, gamma, beta, eps):
    """two-pass LayerNorm over the last axis -> (out, centred, rstd)"""
    v = np.asarray(v, np.float64)
    c = v - v.mean(axis=-1, keepdims=True)
    rstd = 1.0 / np.sqrt((c * c).mean(axis=-1, keepdims=True) + eps)
    return c * rstd * np.asarray(gamma, np.float64) + np.asarray(beta, np.float64), c, rstd


def plane_slots(C, records):
    """-> (slot of channel c's hi half among a pixel's 2C 16-bit slots, distance to its lo half): [hi C | lo C]
    planes, or [C/32][hi 32 | lo 32] records"""
    c = np.arange(C)
    return ((c >> 5) * 64 + (c & 31), 32) if records else (c, C)


# ---- DPT output stage ----
def dpt_pre(x, w, b):
    """y = x w^T + b -> (y, mag)"""
    x, w, b = np.asarray(x, np.float64), np.asarray(w, np.float64), np.asarray(b, np.float64)
    return x @ w.T + b, np.abs(x) @ np.abs(w).T + np.abs(b)


def dpt_act(y, mode):
    """(pts, conf) of y [npix, n_out]: mode 0 exp, mode 1 sign(y) expm1(|y|); conf = 1 + exp(last)"""
    with np.errstate(over="ignore"):
        xyz = y[:, :-1]
        pts = np.exp(xyz) if mode == 0 else np.sign(xyz) * np.expm1(np.abs(xyz))
        return pts, 1.0 + np.exp(y[:, -1])


# ---- patch gather ----
IMAGENET_MEAN = np.array([0.485, 0.456, 0.406], np.float32).astype(np.float64)
IMAGENET_STD = np.array([0.229, 0.224, 0.225], np.float32).astype(np.float64)


def patch_gather(img, p, Kp):
    """img [F, 3, H, W] -> (A, mag) [F * ph * pw, Kp], A[(f, py, px)][c p^2 + dy p + dx] = (img - mean[c]) / std[c]"""
    img = np.asarray(img, np.float64)
    Fr, _, H, W = img.shape
    ph, pw = H // p, W // p
    A, mag = np.zeros((Fr * ph * pw, Kp)), np.zeros((Fr * ph * pw, Kp))
    for f in range(Fr):
        for py in range(ph):
            for px in range(pw):
                r = (f * ph + py) * pw + px
                for c in range(3):
                    t = img[f, c, py * p:(py + 1) * p, px * p:(px + 1) * p].reshape(-1)
                    A[r, c * p * p:(c + 1) * p * p] = (t - IMAGENET_MEAN[c]) / IMAGENET_STD[c]
                    mag[r, c * p * p:(c + 1) * p * p] = (np.abs(t) + IMAGENET_MEAN[c]) / IMAGENET_STD[c]
    return A, mag


# ---- camera head ----
def adaln(xn, x, mod):
    """-> (out, mag); mod [rows, shift | scale | gate]"""
    xn, x, mod = (np.asarray(a, np.float64) for a in (xn, x, mod))
    D = x.shape[1]
    shift, scale, gate = mod[:, :D], mod[:, D:2 * D], mod[:, 2 * D:]
    out = gate * (xn * (1.0 + scale) + shift) + x
    return out, np.abs(gate) * (np.abs(xn) * (1.0 + np.abs(scale)) + np.abs(shift)) + np.abs(x)


def pose_update(delta, pred_pad, first):
    """float32 throughout (one add): -> (pred_pad', act) as float32 arrays"""
    delta = np.asarray(delta, np.float32)
    out = np.array(pred_pad, np.float32, copy=True)
    out[:, :9] = delta if first else out[:, :9] + delta
    act = out[:, :9].copy()
    act[:, 7:] = np.maximum(act[:, 7:], f32(0))
    return out, act


def special_tokens(x, table, S):
    out = np.array(x, copy=True)
    n = table.shape[1]
    for f in range(x.shape[0]):
        out[f, :n] = table[0 if f % S == 0 else 1]
    return out


# ---- track head ----
def avgpool2(x):
    """x [N, H, W, C] -> (out, mag) [N, H/2, W/2, C]"""
    x = np.asarray(x, np.float64)
    _, H, W, _ = x.shape
    Ho, Wo = H // 2, W // 2

    def pool(a):
        a = a[:, :2 * Ho, :2 * Wo]
        return (a[:, 0::2, 0::2] + a[:, 0::2, 1::2] + a[:, 1::2, 0::2] + a[:, 1::2, 1::2]) * 0.25

    return pool(x), pool(np.abs(x))


def _border_taps(p, size):
    """clamped coordinate p (float32 values) -> i0, i1, l (float64, exact: p - floor(p) of an fp32 is an fp32)"""
    p = np.clip(np.asarray(p, np.float32).astype(np.float64), 0.0, size - 1.0)
    i0 = np.floor(p).astype(np.int64)
    return p, i0, np.minimum(i0 + 1, size - 1), p - i0


def sample_border(fmap, coords):
    """fmap [B, H, W, C], coords [B, N, 2] (x, y) fp32 -> (out, mag, slope) [B, N, C]: bilinear, align_corners, border
    padding; slope = |x| |d out / dx| + |y| |d out / dy| of the clamped coordinate, the factor of one coordinate rounding"""
    fmap = np.asarray(fmap, np.float64)
    B, H, W, C = fmap.shape
    N = coords.shape[1]
    out, mag, slope = (np.zeros((B, N, C)) for _ in range(3))
    for b in range(B):
        for n in range(N):
            x, x0, x1, lx = _border_taps(coords[b, n, 0], W)
            y, y0, y1, ly = _border_taps(coords[b, n, 1], H)
            v00, v01, v10, v11 = fmap[b, y0, x0], fmap[b, y0, x1], fmap[b, y1, x0], fmap[b, y1, x1]
            out[b, n] = v00 * (1 - lx) * (1 - ly) + v01 * lx * (1 - ly) + v10 * (1 - lx) * ly + v11 * lx * ly
            mag[b, n] = (np.abs(v00) * (1 - lx) * (1 - ly) + np.abs(v01) * lx * (1 - ly) + np.abs(v10) * (1 - lx) * ly +
                         np.abs(v11) * lx * ly)
            slope[b, n] = (x * np.abs((v01 - v00) * (1 - ly) + (v11 - v10) * ly) +
                           y * np.abs((v10 - v00) * (1 - lx) + (v11 - v01) * lx))
    return out, mag, slope


def pos_embed_table(D, size):
    """[size, D/2]: [sin(p w_k) | cos(p w_k)], w_k = 1 / 10000^(k / (D/4)), float64 values rounded to float32"""
    q = D // 4
    omega = 1.0 / 10000.0 ** (np.arange(q, dtype=np.float64) / q)
    a = np.arange(size, dtype=np.float64)[:, None] * omega[None, :]
    return np.concatenate([np.sin(a), np.cos(a)], axis=1).astype(np.float32).astype(np.float64)


def pos_embed_sample(coords, H, W, D):
    """coords [BN, 2] (x, y) fp32 -> (out, mag, slope) [BN, D]: first D/2 channels from x, last D/2 from y"""
    tx, ty = pos_embed_table(D, W), pos_embed_table(D, H)
    BN = coords.shape[0]
    out, mag, slope = (np.zeros((BN, D)) for _ in range(3))
    for i in range(BN):
        cols = []
        for p, size, tab in ((coords[i, 0], W, tx), (coords[i, 1], H, ty)):
            pc, i0, i1, l = _border_taps(p, size)
            cols.append((tab[i0] * (1 - l) + tab[i1] * l, np.abs(tab[i0]) * (1 - l) + np.abs(tab[i1]) * l,
                         pc * np.abs(tab[i1] - tab[i0])))
        out[i], mag[i], slope[i] = (np.concatenate([cols[0][k], cols[1][k]]) for k in range(3))
    return out, mag, slope


def corr_sample(tgt, fmap, coords, N, S, r, level):
    """The oracle's formulation (tracker_forward): the correlation volume corr = <target, fmap> / sqrt(C) in float64,
    sampled by F.grid_sample(padding_mode="zeros", align_corners=True) on the (2r+1)^2 grid around coords / 2^level,
    delta = stack(meshgrid(d, d, "ij")) added to (x, y): grid row i offsets x, column j offsets y.
    tgt [rows, C], fmap [B S, H, W, C], coords [rows, 2], rows ordered (b, n, s) -> (out, mag) [rows, (2r+1)^2]"""
    tgt, fmap = torch.as_tensor(np.asarray(tgt, np.float64)), torch.as_tensor(np.asarray(fmap, np.float64))
    coords = torch.as_tensor(np.asarray(coords, np.float32).astype(np.float64))
    rows, C = tgt.shape
    _, H, W, _ = fmap.shape
    img = (torch.arange(rows) // (N * S)) * S + torch.arange(rows) % S          # (b, n, s) -> b S + s
    d = torch.linspace(-r, r, 2 * r + 1, dtype=torch.float64)
    delta = torch.stack(torch.meshgrid(d, d, indexing="ij"), dim=-1)
    cl = coords.reshape(rows, 1, 1, 2) / (2 ** level) + delta.view(1, 2 * r + 1, 2 * r + 1, 2)
    grid = cl * torch.tensor([2.0 / max(W - 1, 1), 2.0 / max(H - 1, 1)], dtype=torch.float64) - 1

    def one(t, f):
        corr = torch.einsum("rc,rhwc->rhw", t, f[img]) / math.sqrt(C)
        return F.grid_sample(corr[:, None], grid, align_corners=True, padding_mode="zeros").reshape(rows, -1).numpy()

    return one(tgt, fmap), one(tgt.abs(), fmap.abs())


def flow_embedding(flow, E):
    """get_2d_embedding(flows, E, cat_coords=False) of float32 flows [rows, 2] -> [rows, 2E] float64: angle = flow * div
    in float32 with div = float32(k) * float32(1000 / E), k = 0, 2, ..; sin at even, cos at odd columns, in float64"""
    flow = np.asarray(flow, np.float32)
    div = np.arange(0, E, 2).astype(np.float32) * f32(1000.0 / E)
    out = np.zeros((flow.shape[0], 2 * E))
    for axis in range(2):
        ang = flow[:, axis:axis + 1] * div[None, :]
        assert ang.dtype == np.float32
        out[:, axis * E + 0:(axis + 1) * E:2] = np.sin(ang.astype(np.float64))
        out[:, axis * E + 1:(axis + 1) * E:2] = np.cos(ang.astype(np.float64))
    return out


def track_input(coords, fcorr, tfeat, pos, qrt, S, L, ldx, max_scale):
    """-> (x, mag, is_trig) [rows, ldx]; x = [emb(flow) | flow/ms | flow/ms | fcorr | tfeat] + pos[bn] + qrt[s != 0],
    zero beyond 3L + 4.  flow and flow / max_scale are single float32 operations.  mag = 2 |v| + 2 |pos| + |qrt|: what
    the two roundings of (v + pos) + qrt are relative to, |v + pos| and then |v + pos + qrt|; is_trig marks the sine /
    cosine columns"""
    coords = np.asarray(coords, np.float32)
    rows, D = coords.shape[0], 3 * L + 4
    first = coords.reshape(-1, S, 2)[:, :1].repeat(S, axis=1).reshape(rows, 2)
    flow = coords - first
    fms = flow / f32(max_scale)
    assert flow.dtype == fms.dtype == np.float32
    v = np.concatenate([flow_embedding(flow, L // 2), fms.astype(np.float64), fms.astype(np.float64),
                        np.asarray(fcorr, np.float64), np.asarray(tfeat, np.float64)], axis=1)
    pe = np.repeat(np.asarray(pos, np.float64), S, axis=0)
    q = np.asarray(qrt, np.float64)[(np.arange(rows) % S != 0).astype(np.int64)]
    x, mag, trig = np.zeros((rows, ldx)), np.zeros((rows, ldx)), np.zeros((rows, ldx), bool)
    x[:, :D] = v + pe + q
    mag[:, :D] = 2 * np.abs(v) + 2 * np.abs(pe) + np.abs(q)
    trig[:, :L] = True
    return x, mag, trig


def track_coord_update(coords, delta, query, N, S, stride, want_pred):
    """float32 throughout -> (coords', pred or None): coords += delta[:, :2]; rows s == 0 = query; pred [B, S, N, 2]"""
    coords = np.asarray(coords, np.float32)
    rows = coords.shape[0]
    out = coords + np.asarray(delta, np.float32)[:, :2]
    out = out.reshape(-1, S, 2)
    out[:, 0] = np.asarray(query, np.float32)
    pred = None
    if want_pred:
        pred = np.ascontiguousarray((out * f32(stride)).reshape(-1, N, S, 2).transpose(0, 2, 1, 3))
    return out.reshape(rows, 2), pred


def track_init(q, S, stride):
    """-> (coords [BN, S, 2], qs [BN, 2]) = q * float32(1 / stride), the kernel's form of q / stride (the same value
    for the power-of-two strides the track head uses)"""
    qs = np.asarray(q, np.float32) * (f32(1) / f32(stride))
    return np.repeat(qs[:, None, :], S, axis=1), qs
