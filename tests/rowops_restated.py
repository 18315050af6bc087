"""NumPy restatement of the row-wise kernels (csrc/rowops.hip: LayerNorm, q/k-norm + 2-D RoPE) and of the exact-fp32
attention kernel (csrc/attention_f32.hip), in the style of head_kernels_restated.py.  Three things per operation:

  * a plain float64 reference -- what the GPU tests compare with;
  * an emulation of the kernel's arithmetic in float32, operation by operation in the kernel's order (per-lane serial sums,
    then the xor butterfly; two-pass variance; 32-key tiles with an online softmax).  It exists so that the bounds can be
    checked, and mutants of the kernels shown to break them, without a GPU (test_rowops_cpu.py).  `mutant=` swaps in one
    deliberately wrong step;
  * the per-element error bound, a function of the reference's own quantities in units of U = 2^-24.

The input families and the attention cases of the GPU tests are built here too, so the CPU tests run the emulation on
exactly the inputs the kernels see."""
import numpy as np

from head_kernels_restated import U, bf16_rne_bits, decode16, half_ulp16, layernorm   # noqa: F401  (re-exported for the tests)

f32 = np.float32
_LANES = np.arange(64)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _butterfly(s, offsets=(32, 16, 8, 4, 2, 1)):
    """wave_sum: v += shfl_xor(v, o) for every offset, on the last axis (64 lanes, or 8 for the 8-lane groups); every
    lane ends with the same bits (a + b == b + a)"""
    idx = np.arange(s.shape[-1])
    for o in offsets:
        s = s + s[..., idx ^ o]
    assert s.dtype == np.float32
    return s


def _rsqrt(v):
    """rsqrtf of a float32, correctly rounded (the device's is within a few ulp of it)"""
    return (1.0 / np.sqrt(v.astype(np.float64))).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# LayerNorm with concat and row gather
# ---------------------------------------------------------------------------------------------------------------------
def gather_rows(rows, grp_rows=0, grp_stride=0, grp_off=0):
    """input row of every output row: (r / grp_rows) * grp_stride + grp_off + r % grp_rows, or r"""
    r = np.arange(rows)
    return r // grp_rows * grp_stride + grp_off + r % grp_rows if grp_rows > 0 else r


def ln_input(x, x2=None, rows=None, grp=(0, 0, 0)):
    """the [rows, C] matrix the kernel normalises: x's first C (or, with x2, [x | x2]'s) columns of the gathered rows"""
    x = np.asarray(x)
    idx = gather_rows(x.shape[0] if rows is None else rows, *grp)
    return x[idx] if x2 is None else np.concatenate([x[idx], np.asarray(x2)[idx]], axis=1)


def layernorm_ref(xin, gamma, beta, eps):
    """float64 two-pass LayerNorm of ln_input's matrix -> (ref, centred, rstd); gamma / beta may be None"""
    C = xin.shape[-1]
    return layernorm(xin, np.ones(C) if gamma is None else gamma, np.zeros(C) if beta is None else beta, eps)


def layernorm_tol(xin, cen, rstd, ref, gamma, n=None):
    """fp32 output: (n U max_row|x| + (n + 8) U |cen|) rstd |gamma| + 2 U |ref| with n = ceil(C / 64) + 8.
    First term: the fp32 mean's error, common to the row (it cancels in the variance to second order); second: the
    subtraction, the variance / rsqrt and the scale; third: the gamma multiply and the beta add."""
    xin = np.asarray(xin, np.float64)
    C = xin.shape[-1]
    n = -(-C // 64) + 8 if n is None else n
    g = 1.0 if gamma is None else np.abs(np.asarray(gamma, np.float64))
    xmax = np.abs(xin).max(axis=-1, keepdims=True)
    return (n * U * xmax + (n + 8) * U * np.abs(cen)) * rstd * g + 2 * U * np.abs(ref)


def layernorm_emulate(xin, gamma, beta, eps, kernel="scalar", mutant=None):
    """float32, in the kernel's order.  kernel "scalar" (layernorm_kernel: lane l owns columns l + 64 i) or "vector"
    (layernorm_vec_kernel: lane l owns columns 256 i + 4 l .. + 3, C % 256 == 0).
    mutant: "one_pass" (variance = E[x^2] - mean^2), "half_count" (sums divided by C / 2, the channel count of one
    source of a concat, instead of C)"""
    x = _f32(xin)
    rows, C = x.shape
    div = f32(C // 2 if mutant == "half_count" else C)
    if kernel == "scalar":
        nv = -(-C // 64)
        v = np.zeros((rows, nv * 64), np.float32)
        v[:, :C] = x
        v = v.reshape(rows, nv, 64)                      # v[:, i, l] = x[l + 64 i], zero beyond C
        live = (_LANES[None, :] + 64 * np.arange(nv)[:, None]) < C
        s = np.zeros((rows, 64), np.float32)
        for i in range(nv):
            s = s + v[:, i]
        mean = (_butterfly(s)[:, :1] / div)[:, None, :]
        q = np.zeros((rows, 64), np.float32)
        for i in range(nv):
            if mutant == "one_pass":
                q = q + v[:, i] * v[:, i]
            else:
                d = np.where(live[i], v[:, i] - mean[:, 0], f32(0))
                q = q + d * d
        var = _butterfly(q)[:, :1] / div
        if mutant == "one_pass":
            var = var - mean[:, 0] * mean[:, 0]
        cols = lambda a: a.reshape(rows, nv * 64)[:, :C]      # noqa: E731
    else:
        assert C % 256 == 0
        nv = C // 256
        v = x.reshape(rows, nv, 64, 4)
        inv = f32(1) / div
        s = np.zeros((rows, 64), np.float32)
        for i in range(nv):
            s = s + ((v[:, i, :, 0] + v[:, i, :, 1]) + (v[:, i, :, 2] + v[:, i, :, 3]))
        mean = (_butterfly(s)[:, :1] * inv)[:, None, :, None]
        q = np.zeros((rows, 64), np.float32)
        for i in range(nv):
            d = v[:, i] if mutant == "one_pass" else v[:, i] - mean[:, 0]
            q = q + ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + (d[..., 2] * d[..., 2] + d[..., 3] * d[..., 3]))
        var = _butterfly(q)[:, :1] * inv
        if mutant == "one_pass":
            var = var - mean[:, 0, :, 0] * mean[:, 0, :, 0]
        cols = lambda a: a.reshape(rows, C)                   # noqa: E731
    with np.errstate(invalid="ignore"):
        rstd = _rsqrt(var + f32(eps))
    y = cols((v - mean) * rstd.reshape((rows,) + (1,) * (v.ndim - 1)))
    if gamma is not None:
        y = y * _f32(gamma)
    if beta is not None:
        y = y + _f32(beta)
    assert y.dtype == np.float32
    return y


def ln_family(name, rows, C, seed):
    """the four input families of every LayerNorm path, float32 [rows, C]"""
    g = np.random.default_rng(seed)
    if name == "randn2":
        x = g.standard_normal((rows, C)) * 2.0
    elif name == "mean1e3":
        x = 1e3 + g.standard_normal((rows, C))
    elif name == "constant":
        x = np.repeat(g.standard_normal((rows, 1)) * 3.0, C, axis=1)
    elif name == "scaled":
        x = g.standard_normal((rows, C)) * np.exp2(np.linspace(-10, 10, rows))[:, None]
    else:
        raise KeyError(name)
    return x.astype(np.float32)


LN_FAMILIES = ("randn2", "mean1e3", "constant", "scaled")


def split_hi_lo(y):
    """float32 -> (hi, lo) bf16 patterns of the bf16x3 records: hi = RNE-bf16(y), lo = RNE-bf16(y - hi)"""
    y = _f32(y)
    hb = bf16_rne_bits(y)
    lo = y - decode16(hb, False).astype(np.float32)
    return hb, bf16_rne_bits(lo)


# ---------------------------------------------------------------------------------------------------------------------
# q/k LayerNorm(64) + 2-D RoPE
# ---------------------------------------------------------------------------------------------------------------------
def rope_tables(npos, base=100.0):
    """rope.py:86-117 in float32, the tables the kernels read: [npos, 16] cos, sin"""
    inv_freq = (f32(1) / np.power(f32(base), np.arange(0, 32, 2, dtype=np.float32) / f32(32))).astype(np.float32)
    ang = np.arange(npos, dtype=np.float32)[:, None] * inv_freq[None, :]
    assert ang.dtype == np.float32
    return np.cos(ang).astype(np.float32), np.sin(ang).astype(np.float32)


def qknorm_rope_ref(t, w, b, eps, pos, cos_t, sin_t):
    """float64.  t [tokens, 2 (q | k), heads, 64]; w, b [2, 64] or None (w None: no norm); pos [tokens, 2] (y, x) int or
    None (no RoPE), clamped to the tables; rope.py:154-188: features 0..31 rotate by y, 32..63 by x, d pairs with d +- 16
    inside its half.  -> (ref, tol): tol the fp32 bound:
      tol_t = LayerNorm bound at C = 64 with n = 16 (8 in-lane adds + 3 exchanges, with room), 0 without the norm;
      tol   = tol_t(d) |cos| + tol_t(partner) |sin| + 3 U (|t cos| + |rot sin|)   with RoPE, tol_t without"""
    t = np.asarray(t, np.float64)
    tol_t = np.zeros_like(t)
    if w is not None:
        x = t
        wq = np.asarray(w, np.float64)[None, :, None, :]
        bq = np.zeros_like(wq) if b is None else np.asarray(b, np.float64)[None, :, None, :]
        t, cen, rstd = layernorm(x, wq, bq, eps)
        tol_t = layernorm_tol(x, cen, rstd, t, wq, n=16)
    if pos is None:
        return t, tol_t
    npos = cos_t.shape[0]
    p = np.clip(np.asarray(pos, np.int64), 0, npos - 1)
    c2 = np.concatenate([cos_t, cos_t], axis=-1).astype(np.float64)     # [npos, 32]
    s2 = np.concatenate([sin_t, sin_t], axis=-1).astype(np.float64)

    def one(x, e, pp):
        rot = np.concatenate([-x[..., 16:], x[..., :16]], axis=-1)
        erot = np.concatenate([e[..., 16:], e[..., :16]], axis=-1)
        c, s = c2[pp][:, None, None, :], s2[pp][:, None, None, :]
        return x * c + rot * s, e * np.abs(c) + erot * np.abs(s) + 3 * U * (np.abs(x * c) + np.abs(rot * s))

    (ry, ey), (rx, ex) = one(t[..., :32], tol_t[..., :32], p[:, 0]), one(t[..., 32:], tol_t[..., 32:], p[:, 1])
    return np.concatenate([ry, rx], axis=-1), np.concatenate([ey, ex], axis=-1)


def qknorm_rope_emulate(t, w, b, eps, pos, cos_t, sin_t, kernel="vec", mutant=None):
    """float32 in the kernels' order.  kernel "wave" (qknorm_rope_kernel: one feature per lane, 64-lane butterfly) or
    "vec" (qknorm_rope_vec_kernel and qknorm_rope_bf16_kernel: 8 features per lane, serial, then the 8-lane exchange;
    the bf16 kernel's quad_perm / mirror exchange adds the same pairs).  Same argument shapes as qknorm_rope_ref.
    mutant: "sign" (the negated half is d >= 16), "swap_yx" (features 0..31 rotate by x), "partner8" (d pairs with d +- 8)"""
    t = _f32(t)
    if w is not None:
        wq = _f32(w)[None, :, None, :]
        bq = np.zeros_like(wq) if b is None else _f32(b)[None, :, None, :]
        k = f32(1) / f32(64)
        if kernel == "wave":
            mean = _butterfly(t)[..., :1] * k
            d = t - mean
            var = _butterfly(d * d)[..., :1] * k
        else:
            v = t.reshape(t.shape[:-1] + (8, 8))                  # [.., sub, j]
            s = np.zeros(v.shape[:-1], np.float32)
            for j in range(8):
                s = s + v[..., j]
            mean = (_butterfly(s, (1, 2, 4))[..., :1] * k)
            d = t - mean
            dv = d.reshape(v.shape)
            q = np.zeros(v.shape[:-1], np.float32)
            for j in range(8):
                q = q + dv[..., j] * dv[..., j]
            var = _butterfly(q, (1, 2, 4))[..., :1] * k
        t = d * _rsqrt(var + f32(eps)) * wq + bq
    if pos is not None:
        npos = cos_t.shape[0]
        p = np.clip(np.asarray(pos, np.int64), 0, npos - 1)
        sect, dd = _LANES >> 5, _LANES & 31
        if mutant == "swap_yx":
            sect = 1 - sect
        pp = p[:, sect]                                           # [tokens, 64]
        c = _f32(cos_t)[pp, dd & 15][:, None, None, :]
        s = _f32(sin_t)[pp, dd & 15][:, None, None, :]
        other = t[..., _LANES ^ (8 if mutant == "partner8" else 16)]
        neg = (dd >= 16) if mutant == "sign" else (dd < 16)
        rot = np.where(neg, -other, other)
        t = t * c + rot * s
    assert t.dtype == np.float32
    return t


QK_SHAPES = [(1, 1), (3, 1), (5, 3), (33, 2), (201, 3)]


def qk_case(tokens, heads, npos, seed=0, bf16=False):
    """head vectors with a per-head offset of 8, q and k weights from different seeds, y and x differing per token, and the
    positions -3 and npos + 5 among them"""
    g = np.random.default_rng(500 + tokens + heads + seed)
    t = g.standard_normal((tokens, 2, heads, 64)) + 8.0 * np.arange(1, heads + 1)[None, None, :, None]
    t = t.astype(np.float32)
    if bf16:
        t = decode16(split_hi_lo(t)[0], False).astype(np.float32)
    w = (1.0 + 0.2 * g.standard_normal((2, 64))).astype(np.float32)
    b = (0.1 * g.standard_normal((2, 64))).astype(np.float32)
    pos = np.stack([(np.arange(tokens) * 7 + 1) % npos, (np.arange(tokens) * 5 + 3) % npos], axis=1).astype(np.int32)
    pos[0] = (-3, npos + 5)
    return t, w, b, pos


# ---------------------------------------------------------------------------------------------------------------------
# fp32 attention on strided streams
# ---------------------------------------------------------------------------------------------------------------------
def gather_stream(buf, off, strides, batch, batch_inner, heads, seq, hd):
    """flat buffer -> [batch, heads, seq, hd]: element (g, h, t, d) at off + go strides[3] + gi strides[2] + h strides[1] +
    t strides[0] + d, g = go batch_inner + gi (batch_inner 0: gi = g)"""
    return np.asarray(buf).reshape(-1)[stream_index(off, strides, batch, batch_inner, heads, seq, hd)]


def stream_index(off, strides, batch, batch_inner, heads, seq, hd):
    g = np.arange(batch)
    go, gi = (g // batch_inner, g % batch_inner) if batch_inner > 0 else (0 * g, g)
    return (off + (go * strides[3] + gi * strides[2])[:, None, None, None] + (np.arange(heads) * strides[1])[None, :, None, None] +
            (np.arange(seq) * strides[0])[None, None, :, None] + np.arange(hd)[None, None, None, :])


def attention_ref(q, k, v, scale):
    """float64 softmax(scale q k^T) v on [.., seq, hd] arrays"""
    q, k, v = (np.asarray(a, np.float64) for a in (q, k, v))
    s = scale * (q @ np.swapaxes(k, -1, -2))
    p = np.exp(s - s.max(axis=-1, keepdims=True))
    return (p / p.sum(axis=-1, keepdims=True)) @ v


def _fma(a, b, c):
    """float32 fma: the product of two float32 is exact in float64"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def attention_emulate(q, k, v, scale, mutant=None):
    """float32 in attn_f32_kernel's order, on [.., seq, hd] arrays: q * scale; per 32-key tile the score chain
    s = fma(k[d], q[d], s) with d alternating between the two lane halves (t, HD/2 + t); keys >= seq_k masked; running
    max, alpha = exp(m_old - m_new), p = exp(s - m_new); each lane half sums its 16 keys serially and the halves meet at
    the end; o = o alpha, then fma(v[key], p[key], o) over the tile's keys in register order; out = o * (1 / l).
    mutant: "no_alpha" (the rescale of o and l by alpha omitted), "mask_off_by_one" (the key at seq_k, a zero row of the
    staged tile, admitted)"""
    q, k, v = _f32(q), _f32(k), _f32(v)
    hd, sq, sk = q.shape[-1], q.shape[-2], k.shape[-2]
    HD = 64 if hd <= 64 else 128
    HDH = HD // 2
    lead = q.shape[:-2]
    qs = np.zeros(lead + (sq, HD), np.float32)
    qs[..., :hd] = q * f32(scale)
    nkt = (sk + 31) // 32
    kp = np.zeros(lead + (nkt * 32, HD), np.float32)
    vp = np.zeros(lead + (nkt * 32, hd), np.float32)
    kp[..., :sk, :hd], vp[..., :sk, :] = k, v
    o = np.zeros(lead + (sq, hd), np.float32)
    m = np.full(lead + (sq,), -np.inf, np.float32)
    lsum = np.zeros(lead + (sq, 2), np.float32)                   # per lane half
    regkeys = np.array([(r & 3) + 8 * (r >> 2) for r in range(16)])
    limit = sk + 1 if mutant == "mask_off_by_one" else sk
    for kt in range(nkt):
        kk, vv = kp[..., kt * 32:kt * 32 + 32, :], vp[..., kt * 32:kt * 32 + 32, :]
        s = np.zeros(lead + (sq, 32), np.float32)
        for t in range(HDH):
            for d in (t, HDH + t):
                if d < hd:                                        # beyond head_dim both operands are zero: s unchanged
                    s = _fma(kk[..., None, :, d], qs[..., :, None, d], s)
        s = np.where(kt * 32 + np.arange(32) >= limit, f32(-np.inf), s)
        mnew = np.maximum(m, s.max(axis=-1))
        with np.errstate(invalid="ignore"):
            alpha = np.exp(m - mnew)
        alpha = np.where(np.isneginf(m), f32(0), alpha).astype(np.float32)
        m = mnew
        p = np.exp(s - mnew[..., None]).astype(np.float32)
        psum = np.zeros(lead + (sq, 2), np.float32)
        for r in regkeys:
            psum = psum + np.stack([p[..., r], p[..., r + 4]], axis=-1)
        if mutant == "no_alpha":
            alpha = np.ones_like(alpha)
        lsum = lsum * alpha[..., None] + psum
        o = o * alpha[..., None]
        for r in regkeys:
            for key in (r, r + 4):
                o = _fma(vv[..., None, key, :], p[..., :, key, None], o)
    inv = f32(1) / (lsum[..., 0] + lsum[..., 1])
    out = o * inv[..., None]
    assert out.dtype == np.float32
    return out


def attention_tol(q, k, v, scale, unit_variance=True):
    """-> (ref float64, tol scalar, emulation error): tol = 16 x the worst error of the fp32 emulation against float64 on
    these inputs, at least 16 U max|v|, and for unit-variance inputs at most the 2e-5 of the older tests.  16 x covers a
    device expf a couple of ulp off where the CPU's is half an ulp, and another summation order inside the MFMA chain."""
    ref = attention_ref(q, k, v, scale)
    err = float(np.abs(attention_emulate(q, k, v, scale).astype(np.float64) - ref).max())
    tol = max(16 * err, 16 * U * float(np.abs(np.asarray(v, np.float64)).max()))
    return ref, (min(tol, 2e-5) if unit_variance else tol), err


def attention_softmax_case(name, seq_q=5, seq_k=40, hd=64, seed=0):
    """(q, k, v, unit_variance) float32 [1, 1, seq, hd] of the softmax edge cases; scores are q k / sqrt(hd).
    unit_variance (the 2e-5 cap of attention_tol applies) only where q, k and v are all plain randn"""
    g = np.random.default_rng(7000 + seed)
    q, k, v = (g.standard_normal((1, 1, n, hd)).astype(np.float32) for n in (seq_q, seq_k, seq_k))
    unit = True
    if name == "scores_x4":
        q, unit = q * f32(4), False
    elif name in ("spike_last_tile", "spike_first_tile"):
        # key j = 3 q_0 direction, so that query 0 scores it ~ 30 nats above the rest (|q_0|^2 ~ hd, score 3.75 sqrt(hd))
        j = seq_k - 2 if name == "spike_last_tile" else 1
        k[0, 0, j] = q[0, 0, 0] * f32(30.0 * np.sqrt(hd) / float(np.dot(q[0, 0, 0].astype(np.float64), q[0, 0, 0])))
        unit = False
    elif name == "equal_scores":
        k[...] = k[:, :, :1]
    elif name == "large_v_row":
        v[0, 0, seq_k // 2] *= f32(1e4)
        unit = False
    elif name != "plain":
        raise KeyError(name)
    return q, k, v, unit


SOFTMAX_CASES = ("plain", "scores_x4", "spike_last_tile", "spike_first_tile", "equal_scores", "large_v_row")
