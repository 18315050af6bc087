"""Float64 restatement of the small-batch VideoPose3D streaming layers (csrc/vp3d_stream.hip, csrc/vp3d_dense.hip),
numpy only, written from the layout and the arithmetic the two file headers and include/skimi.h document -- not from
the library's own weight packer.

Operands.  A value x (fp32) travels as two bf16 halves, hi = bf16(x) and lo = bf16(x - hi), round to nearest even (the
difference is exact in fp32).  Records are fragment-major,
    [row tile of 16][K slice of 32][hi | lo][kg 0..3][row 0..15][8 elements],
the register image of a 16 x 32 MFMA operand.  The kernels keep three of the four products of (Whi + Wlo)(Xhi + Xlo):
    Whi Xhi + Whi Xlo + Wlo Xhi                                                    (the lo x lo term is dropped).

Two references per layer.  A: the exact (float64) sum of those three products on the split operands -- what the kernel
computes up to the order of its fp32 additions.  B: the plain float64 product of the unsplit fp32 operands -- what the
layer means.  Both come with the sums of absolute values their error bounds are made of.
"""
from __future__ import annotations

import numpy as np

U = 2.0 ** -24        # unit roundoff of fp32
UB = 2.0 ** -8        # unit roundoff of bf16 (8 significant bits)


# ---- bf16 ------------------------------------------------------------------------------------------------------
def bf16_bits(x):
    """fp32 -> the 16 bits of bf16(x), round to nearest, ties to even (finite inputs)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    lsb = (u >> np.uint64(16)) & np.uint64(1)
    return ((u + np.uint64(0x7FFF) + lsb) >> np.uint64(16)).astype(np.uint16)


def bf16_value(bits):
    """the 16 bits of a bf16 -> its value as fp32"""
    return (np.asarray(bits).astype(np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def split(x):
    """x (fp32) -> (hi, lo), fp32 arrays holding bf16 values: hi = bf16(x), lo = bf16(x - hi)"""
    x = np.asarray(x, dtype=np.float32)
    hi = bf16_value(bf16_bits(x))
    lo = bf16_value(bf16_bits(x - hi))      # x - hi is exact in fp32 (Sterbenz / a 16-bit remainder)
    return hi, lo


# ---- fragment-major records ------------------------------------------------------------------------------------
def pack(x, rows_pad=None):
    """x [rows, K] fp32 (K % 32 == 0) -> records [tiles, K / 32, 2, 4, 16, 8] uint16; rows up to the tile (or
    rows_pad, a multiple of 16) are zero."""
    x = np.asarray(x, dtype=np.float32)
    rows, K = x.shape
    assert K % 32 == 0
    T = -(-(rows_pad or rows) // 16)
    full = np.zeros((T * 16, K), np.float32)
    full[:rows] = x
    hi, lo = split(full)
    rec = np.empty((T, K // 32, 2, 4, 16, 8), np.uint16)
    for h, plane in enumerate((hi, lo)):
        # [T, 16 rows, S, 4 kg, 8] -> [T, S, kg, row, 8]
        rec[:, :, h] = bf16_bits(plane).reshape(T, 16, K // 32, 4, 8).transpose(0, 2, 3, 1, 4)
    return rec


def unpack(rec, rows, K):
    """records (any shape / integer dtype of the right size) -> (hi, lo) fp32 [rows, K]"""
    T = -(-rows // 16)
    rec = np.asarray(rec).view(np.uint16).reshape(-1)[: T * (K // 32) * 1024].reshape(T, K // 32, 2, 4, 16, 8)
    out = []
    for h in range(2):
        plane = rec[:, :, h].transpose(0, 3, 1, 2, 4).reshape(T * 16, K)
        out.append(bf16_value(plane)[:rows].copy())
    return out[0], out[1]


def record_index(row, k, K):
    """16-bit index of the hi half of element (row, k); the lo half is 512 further (include/skimi.h)"""
    return ((row // 16) * (K // 32) + k // 32) * 1024 + ((k % 32 // 8) * 16 + row % 16) * 8 + k % 8


# ---- layers ----------------------------------------------------------------------------------------------------
def _windows(X, taps, dil):
    """X [B, Lin, C] -> [B, Lout, taps * C], window l = rows l, l + dil, ... (tap-major K)"""
    B, Lin, C = X.shape
    Lout = Lin - (taps - 1) * dil
    return np.concatenate([X[:, t * dil: t * dil + Lout] for t in range(taps)], axis=2)


def _contract(Wm, Xw, bias, relu, resid):
    """Wm [N, K] fp32, Xw [B, Lout, K] fp32 -> dict of float64 [B, Lout, N] arrays:
    A, B the two references (bias, ReLU and residual applied), SA = sum |kept terms| + |bias| + |resid|,
    SB = sum |w| |x| (the unsplit operands)."""
    Wm = np.asarray(Wm, np.float32)
    Xw = np.asarray(Xw, np.float32)
    wh, wl = (a.astype(np.float64) for a in split(Wm))
    xh, xl = (a.astype(np.float64) for a in split(Xw))
    w64, x64 = Wm.astype(np.float64), Xw.astype(np.float64)
    A = xh @ wh.T + xl @ wh.T + xh @ wl.T
    SA = np.abs(xh) @ np.abs(wh).T + np.abs(xl) @ np.abs(wh).T + np.abs(xh) @ np.abs(wl).T
    Bv = x64 @ w64.T
    SB = np.abs(x64) @ np.abs(w64).T
    b64 = np.asarray(bias, np.float64)
    A, Bv = A + b64, Bv + b64
    SA = SA + np.abs(b64)
    if relu:
        A, Bv = np.maximum(A, 0.0), np.maximum(Bv, 0.0)
    if resid is not None:
        r = np.asarray(resid, np.float64)
        A, Bv, SA = A + r, Bv + r, SA + np.abs(r)
    return {"A": A, "B": Bv, "SA": SA, "SB": SB}


def conv(W, X, bias, dil=1, relu=True, resid=None, resid_off=0):
    """The dilated conv of the chain.  W [N, taps, C], X [B, Lin, C], bias [N]; resid [B, resid_L, N] or None: output row
    (b, l) adds resid[b, l + resid_off] after the ReLU (x = res + relu(bn(conv(x))), model.py:129-135)."""
    W = np.asarray(W, np.float32)
    N, taps, C = W.shape
    Xw = _windows(np.asarray(X, np.float32), taps, dil)
    r = None
    if resid is not None:
        r = np.asarray(resid)[:, resid_off: resid_off + Xw.shape[1]]
    return _contract(W.reshape(N, taps * C), Xw, bias, relu, r)


def contract_rows(W, X, bias, dil, relu, rows):
    """conv() without a residual for the output rows `rows` (indices into the B * Lout rows) only"""
    W = np.asarray(W, np.float32)
    N, taps, C = W.shape
    Xw = _windows(np.asarray(X, np.float32), taps, dil)
    return _contract(W.reshape(N, taps * C), Xw.reshape(-1, taps * C)[rows], bias, relu, None)


def window_conv(W, X, bias):
    """The dense model's wide conv: dilation 1, ReLU, no residual"""
    return conv(W, X, bias, 1, True)


def expand(W, X, bias):
    """expand_conv: W [C, taps, Cin], X [B, Lin, Cin] read directly (row l's K vector = the taps * Cin consecutive floats
    from row l), ReLU.  Reference A splits x as the MFMA kernel does in registers."""
    return conv(W, X, bias, 1, True)


# ---- the TemporalModel forward, plain and dense, with a propagated error bound ----------------------------------
def pads(filter_widths, causal):
    pad, shift = [filter_widths[0] // 2], [filter_widths[0] // 2 if causal else 0]
    nd = filter_widths[0]
    for fw in filter_widths[1:]:
        pad.append((fw - 1) * nd // 2)
        shift.append(fw // 2 * nd if causal else 0)
        nd *= fw
    return pad, shift


def receptive_field(filter_widths):
    return 1 + 2 * sum(pads(filter_widths, False)[0])


def _fold(sd, conv_key, bn_key):
    """BN(eval) folded into the conv in float64: W'[co][t][ci], b'[co], and |beta| + |mean s| (the bias's own terms)"""
    w = sd[conv_key + ".weight"].double().numpy()                 # [co, ci, t]
    g, be = sd[bn_key + ".weight"].double().numpy(), sd[bn_key + ".bias"].double().numpy()
    mu, var = sd[bn_key + ".running_mean"].double().numpy(), sd[bn_key + ".running_var"].double().numpy()
    s = g / np.sqrt(var + 1e-5)
    return w.transpose(0, 2, 1) * s[:, None, None], be - mu * s, np.abs(be) + np.abs(mu * s)


def forward(sd, x, filter_widths, causal=False, dense=False, with_bound=False):
    """x [B, L, J, F] -> [B, L - rf + 1, J_out, 3] in float64 (model.py:79-138, eval mode).

    with_bound: also the bound on |kernel - this| that the per-layer bounds of the streaming kernels give, propagated:
    with E the bound on a layer's input, T = |W'| (|x| + E) and n = 3 K + 27 additions on an output's longest path
    (tests/test_vp3d_stream_gpu.py, "random data"),
        E_out = |W'| E  +  (4 u + 1.01 n u + 3 * 2^-16) T  +  (n + 4) u (|beta| + |mean s|)  +  E_resid,
    where 4 u covers the fp32 fold of BN into W' (s = g / sqrt(var + eps): three roundings, the product a fourth),
    1.01 n u the fp32 accumulation of the kept terms (their absolute sum is within 1 + 2^-7 of T), 3 * 2^-16 the bf16x3
    split of both operands, and ReLU is 1-Lipschitz."""
    x = np.asarray(x, np.float64)
    B, L = x.shape[:2]
    h = x.reshape(B, L, -1)
    E = np.zeros_like(h)
    pad, shift = pads(filter_widths, causal)

    def layer(h, E, W, b, babs, dil, relu, fold_u):
        N, taps, C = W.shape
        hw, Ew = _windows(h, taps, dil), _windows(E, taps, dil)
        Wm = W.reshape(N, taps * C)
        y = hw @ Wm.T + b
        K = -(-taps * C // 32) * 32
        n = 3 * K + 27
        T = (np.abs(hw) + Ew) @ np.abs(Wm).T
        Eo = Ew @ np.abs(Wm).T + (fold_u * U + 1.01 * n * U + 3 * 2.0 ** -16) * T + (n + fold_u) * U * babs
        return (np.maximum(y, 0.0) if relu else y), Eo

    W, b, babs = _fold(sd, "expand_conv", "expand_bn")
    h, E = layer(h, E, W, b, babs, 1, True, 4)
    nd = 1
    for i in range(1, len(filter_widths)):
        nd *= filter_widths[i - 1]
        lo, hi_ = pad[i] + shift[i], h.shape[1] - pad[i] + shift[i]
        res, Eres = h[:, lo:hi_], E[:, lo:hi_]
        W, b, babs = _fold(sd, f"layers_conv.{2 * (i - 1)}", f"layers_bn.{2 * (i - 1)}")
        assert W.shape[1] == (2 * pad[i] + 1 if dense else filter_widths[i])
        dil = 1 if dense else nd
        h, E = layer(h, E, W, b, babs, dil, True, 4)
        W, b, babs = _fold(sd, f"layers_conv.{2 * (i - 1) + 1}", f"layers_bn.{2 * (i - 1) + 1}")
        h, E = layer(h, E, W, b, babs, 1, True, 4)
        h, E = h + res, E + Eres + U * (np.abs(h) + np.abs(res))
    W = sd["shrink.weight"].double().numpy().transpose(0, 2, 1)
    bs = sd["shrink.bias"].double().numpy()
    h, E = layer(h, E, W, bs, np.abs(bs), 1, False, 0)
    J = bs.shape[0] // 3
    if with_bound:
        return h.reshape(B, -1, J, 3), E.reshape(B, -1, J, 3)
    return h.reshape(B, -1, J, 3)
