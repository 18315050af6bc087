"""GPU: LayerNorm, q/k-norm + RoPE (csrc/rowops.hip) and the exact-fp32 attention kernel (csrc/attention_f32.hip) on every
launch path the forward takes, against the float64 references of rowops_restated.py.

Outputs sit in `Guarded` buffers (0xFF prefill, 256 guard bytes on both sides) as in test_head_kernels_gpu.py, whose helpers
are used here.  Every LayerNorm / q/k-norm tolerance is a per-element bound built from the reference's own quantities
(rowops_restated.layernorm_tol, qknorm_rope_ref); the attention tolerance is 16 x the error of the float32 emulation of the
kernel on the case's own inputs (rowops_restated.attention_tol).  test_rowops_cpu.py shows without a GPU that the
emulations meet these bounds and that mutants of them do not.  The worst error / bound per key is printed
(profiles/rowops_tests.md; SKIMI_ROWOPS_RATIOS=<file> writes them as JSON)."""
import json
import os

import numpy as np
import pytest
import torch

import head_kernels_restated as HR
import rowops_restated as R
import test_head_kernels_gpu as HK
from skiing_analysis_pytorch_amd import _lib, ops
from test_head_kernels_gpu import Guarded, _bits16, _check, _check_hi_lo, _np

pytestmark = pytest.mark.gpu

U = R.U
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
PREFIXES = ("ln ", "qk ", "attn ")      # this file's keys in the shared worst-ratio record
EMU_ERR = {}                            # attention: the emulation error each tolerance was taken from


@pytest.fixture(scope="module", autouse=True)
def _report_ratios():
    yield
    mine = {k: v for k, v in HK.RATIOS.items() if k.startswith(PREFIXES)}
    for k in sorted(mine):
        print(f"worst error / bound  {k:44s} {mine[k]:.3f}" + (f"   (emulation error {EMU_ERR[k]:.2e})" if k in EMU_ERR else ""))
    path = os.environ.get("SKIMI_ROWOPS_RATIOS")
    if path:
        with open(path, "w") as f:
            json.dump({"ratios": mine, "attention_emulation_error": EMU_ERR}, f, indent=1, sort_keys=True)


def _guarded(dtype, shape, off=0):
    """(Guarded, tensor of `shape`): the tensor starts `off` bytes past a 256-byte aligned address, 0xFF everywhere"""
    n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    g = Guarded(torch.uint8, (256 + off + n,))
    g.lo = (-g.t.data_ptr()) % 256 + off
    g.hi = g.lo + n
    t = g.t[g.lo:g.hi].view(dtype).view(*shape)
    assert t.data_ptr() % 256 == off
    return g, t


def _check_guards(g):
    g.check()
    assert (g.t[:g.lo] == 0xFF).all() and (g.t[g.hi:] == 0xFF).all(), "bytes next to a (misaligned) output were written"


def _at(a, off=0, dtype=torch.float32):
    """host array -> device tensor starting `off` bytes past a 256-byte aligned address (None stays None)"""
    if a is None:
        return None
    src = torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    _, t = _guarded(dtype, src.shape, off)
    t.copy_(src)
    return t


def _strided(a, ld, off=0):
    """float32 [N, C] -> device view [N, C] on row stride ld, the padding columns NaN"""
    full = np.full((a.shape[0], ld), np.nan, np.float32)
    full[:, :a.shape[1]] = a
    return _at(full, off)[:, :a.shape[1]]


# ------------------------------------------------------------------------------------------------------------------
# LayerNorm
# ------------------------------------------------------------------------------------------------------------------
def _ln(key, x32, *, x2=None, gamma=True, beta=True, out="f32", ldx=None, ldo=None, rows=None, grp=(0, 0, 0), off_x=0, off_g=0,
        off_o=0, eps=1e-5):
    """one launch through ops.layernorm's strided form, checked against float64 on the values the buffers hold"""
    N, Cs = x32.shape
    C = Cs * (2 if x2 is not None else 1)
    if rows is None:
        rows = N // grp[1] * grp[0] if grp[0] else N
    g = np.random.default_rng(1000 + C)
    gam32 = (1.0 + 0.5 * g.standard_normal(C)).astype(np.float32) if gamma else None
    bet32 = g.standard_normal(C).astype(np.float32) if beta else None
    x = _strided(x32, ldx or Cs, off_x)
    x2d = _strided(x2, ldx or Cs) if x2 is not None else None
    gam, bet = _at(gam32, off_g), _at(bet32)
    xin = R.ln_input(x32, x2, rows, grp)
    assert np.isfinite(xin).all()
    ref, cen, rstd = R.layernorm_ref(xin, gam32, bet32, eps)
    tol = R.layernorm_tol(xin, cen, rstd, ref, gam32)
    kw = dict(x2=x2d, rows=rows, grp_rows=grp[0], grp_stride=grp[1], grp_off=grp[2])
    if out == "records":
        gb, o = _guarded(torch.int16, (rows * 2 * C + 128,))
        ops.layernorm(x, gam, bet, eps, out_dtype="records", out=o, **kw)
        _check_guards(gb)                                             # the byte behind the zero page is untouched
        bits = _bits16(o)
        assert not bits[rows * 2 * C:].any(), "the 256 bytes behind the records must be zero"
        slot, lo_off = HR.plane_slots(C, True)
        _check_hi_lo(key, bits[:rows * 2 * C].reshape(rows, 2 * C), slot, lo_off, ref, tol)
        # bit for bit the records of the fp32 result of the same launch: out_dtype is a run-time branch behind the last
        # fp32 operation of layernorm_vec_kernel, so both stores start from the same y, and split_records_kernel rounds it
        # as the records branch does (hi = bf16(y), lo = bf16(y - hi); the library is built without contraction)
        y = ops.layernorm(x, gam, bet, eps, out_dtype=torch.float32, **kw)
        assert torch.equal(o[:rows * 2 * C], ops.split_records(y).view(torch.int16).reshape(-1)), \
            "records differ from split_records(fp32 LayerNorm)"
        return
    ldo = ldo or C
    gb, o = _guarded(DT[out], (rows, ldo), off_o)
    ops.layernorm(x, gam, bet, eps, out=o[:, :C], **kw)
    _check_guards(gb)
    if ldo > C:
        assert (o[:, C:].contiguous().view(torch.uint8) == 0xFF).all(), "padding columns of the output were written"
    if out != "f32":
        tol = tol + R.half_ulp16(ref, out == "f16")
    _check(key, _np(o[:, :C]), ref, tol)


@pytest.mark.parametrize("family", R.LN_FAMILIES)
@pytest.mark.parametrize("C", [256, 512, 768, 1024, 1536, 2048])
def test_layernorm_vector(C, family):
    """layernorm_vec_kernel<NV>, one case per NV"""
    _ln(f"ln vector {family}", R.ln_family(family, 37, C, 11 * C))


@pytest.mark.parametrize("family", R.LN_FAMILIES)
@pytest.mark.parametrize("C", [1280, 1792, 1, 2, 63, 64, 65, 128, 129, 388, 516, 1088, 2047])
def test_layernorm_scalar_by_shape(C, family):
    """layernorm_kernel<MAXV>: the C / 256 in {5, 7} fall-through of the vector switch, and every MAXV (2, 8, 16, 32) at
    its edges (C <= 128, <= 512, <= 1024, <= 2048)"""
    _ln(f"ln scalar {family}", R.ln_family(family, 37, C, 11 * C))


@pytest.mark.parametrize("family", R.LN_FAMILIES)
@pytest.mark.parametrize("how", ["aligned", "x+4", "gamma+4", "out+4", "ldx=C+2"])
def test_layernorm_scalar_fallback(how, family):
    """C = 512: the vector kernel, and the scalar kernel reached through a 4-byte misaligned operand or a row stride
    that is no multiple of 4 -- the same data, each within the bound (they need not be equal)"""
    kw = {"aligned": {}, "x+4": dict(off_x=4), "gamma+4": dict(off_g=4), "out+4": dict(off_o=4), "ldx=C+2": dict(ldx=514)}[how]
    _ln(f"ln C=512 {how}", R.ln_family(family, 37, 512, 77), **kw)


@pytest.mark.parametrize("family", R.LN_FAMILIES)
@pytest.mark.parametrize("C", [512, 130])
@pytest.mark.parametrize("rows", [1, 2, 3, 4, 5])
def test_layernorm_row_tail_strides_affine(rows, C, family):
    """the 4-rows-per-workgroup tail, ldx = C + 8 and ldo = C + 12, gamma / beta present or null independently"""
    x = R.ln_family(family, rows, C, 13 * C + rows)
    for gamma in (True, False):
        for beta in (True, False):
            _ln(f"ln tail {'vector' if C == 512 else 'scalar'}", x, gamma=gamma, beta=beta, ldx=C + 8, ldo=C + 12)


@pytest.mark.parametrize("family", R.LN_FAMILIES)
@pytest.mark.parametrize("out", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("C", [1024, 388])
def test_layernorm_out_types(C, out, family):
    """16-bit output: the fp32 bound plus half a unit in the last place of the format at the reference"""
    _ln(f"ln {out} {'vector' if C == 1024 else 'scalar'}", R.ln_family(family, 9, C, 17 * C), out=out, ldo=C + 12)


@pytest.mark.parametrize("family", R.LN_FAMILIES)
@pytest.mark.parametrize("C", [256, 1024, 2048])
def test_layernorm_records(C, family):
    for rows in (1, 3, 37):
        _ln(f"ln records {family}", R.ln_family(family, rows, C, 19 * C + rows), out="records")


def test_layernorm_records_rejected():
    """C % 256 != 0, a buffer that is not 128-byte aligned, and the scalar fall-back: an error code, nothing written"""
    def refused(C, out_off=0, **kw):
        x = _strided(R.ln_family("randn2", 4, C, 5), kw.pop("ldx", C), kw.pop("off_x", 0))
        gb, o = _guarded(torch.int16, (4 * 2 * C + 128,), out_off)
        with pytest.raises(_lib.SkimiError, match="records output"):
            ops.layernorm(x, None, None, 1e-5, out_dtype="records", out=o)
        torch.cuda.synchronize()
        _check_guards(gb)
        assert (gb.t == 0xFF).all()

    refused(384)
    refused(512, out_off=64)
    refused(512, off_x=4)
    refused(512, ldx=514)
    refused(1280)          # C / 256 = 5 has no vector kernel


@pytest.mark.parametrize("family", R.LN_FAMILIES)
@pytest.mark.parametrize("C", [130, 768, 512, 2048])
def test_layernorm_concat(C, family):
    """[x | x2]: odd halves (65), halves of 384 (scalar kernel), and the vector kernel; the two sources come from different
    seeds and have different means, so a swapped or repeated half shows"""
    xa, xb = R.ln_family(family, 37, C // 2, 5 * C), R.ln_family(family, 37, C // 2, 5 * C + 1) + np.float32(0.75)
    _ln(f"ln concat {'vector' if C in (512, 2048) else 'scalar'}", xa, x2=xb)


def _dpt_rows(C, family, F=3, P=11, off=5):
    """F frames of P tokens; the first `off` of each frame (the special tokens the DPT heads drop) are NaN"""
    x = R.ln_family(family, F * P, C, 23 * C)
    x.reshape(F, P, C)[:, :off] = np.nan
    return x


@pytest.mark.parametrize("family", R.LN_FAMILIES)
@pytest.mark.parametrize("C", [128, 512])
@pytest.mark.parametrize("rows", [18, 14, 17])
def test_layernorm_gather(rows, C, family):
    """the DPT shape in small: grp_off = 5, grp_rows = 6, grp_stride = 11; rows = 14 and 17 end inside a group and
    inside a workgroup"""
    _ln(f"ln gather {'vector' if C == 512 else 'scalar'}", _dpt_rows(C, family), rows=rows, grp=(6, 11, 5))


@pytest.mark.parametrize("family", R.LN_FAMILIES)
def test_layernorm_gather_concat_records(family):
    """the launch of the DPT heads in parity mode (vggt_dpt.hip): gather + [frame | global] concat + records, C = 512"""
    xa, xb = _dpt_rows(256, family), _dpt_rows(256, family) * np.float32(0.5) + np.float32(0.75)
    for rows in (18, 14):
        _ln("ln gather+concat records", xa, x2=xb, rows=rows, grp=(6, 11, 5), out="records")
        _ln("ln gather+concat f32", xa, x2=xb, rows=rows, grp=(6, 11, 5))


# ------------------------------------------------------------------------------------------------------------------
# q/k-norm + RoPE
# ------------------------------------------------------------------------------------------------------------------
QK_VARIANTS = {"norm+rope": (True, True, True), "norm only": (True, True, False), "rope only": (False, False, True),
               "null bias": (True, False, True)}
# kernel -> (dtype, byte offset of qkv, [(variant, npos)]): each selected the way qknorm_rope_launch selects it
QK_PATHS = {
    "bf16 fast": ("bf16", 0, [("norm+rope", 38), ("norm+rope", 384), ("null bias", 38)]),
    "vector f32": ("f32", 0, [(v, 38) for v in sorted(QK_VARIANTS)] + [("norm+rope", 384), ("norm+rope", 385)]),
    "vector bf16": ("bf16", 0, [("norm only", 38), ("rope only", 38), ("norm+rope", 385), ("null bias", 385)]),
    "scalar f32": ("f32", 4, [(v, 38) for v in sorted(QK_VARIANTS)] + [("norm+rope", 384), ("norm+rope", 385)]),
    "scalar bf16": ("bf16", 2, [(v, 38) for v in sorted(QK_VARIANTS)] + [("norm+rope", 384), ("norm+rope", 385)]),
}
_TABLES = {}


def _rope(npos):
    if npos not in _TABLES:
        c, s = R.rope_tables(npos)
        _TABLES[npos] = (c, s, _at(c), _at(s))
    return _TABLES[npos]


def _qk(path, tokens, heads, variant, npos):
    dt, off, _ = QK_PATHS[path]
    norm, bias, rope = QK_VARIANTS[variant]
    cos_t, sin_t, cos_d, sin_d = _rope(npos)
    t32, w, b, pos = R.qk_case(tokens, heads, npos)
    v32 = np.random.default_rng(tokens).standard_normal((tokens, 1, heads, 64)).astype(np.float32)
    src = torch.from_numpy(np.concatenate([t32, v32], axis=1)).to(DT[dt])           # [tokens, 3, heads, 64]
    held = src.double().numpy()
    gb, qkv = _guarded(DT[dt], (tokens, 3 * heads * 64), off)
    qkv.copy_(src.reshape(tokens, -1))
    wd = [_at(w[0]), _at(b[0]) if bias else None, _at(w[1]), _at(b[1]) if bias else None] if norm else [None] * 4
    pos_d = _at(pos, dtype=torch.int32) if rope else None
    ops.qknorm_rope_(qkv, heads, *wd, 1e-5, pos_d, cos_d, sin_d)
    _check_guards(gb)
    got = qkv.reshape(tokens, 3, heads, 64)
    assert torch.equal(got[:, 2].cpu(), src[:, 2]), "v must come back bit for bit"
    ref, tol = R.qknorm_rope_ref(held[:, :2], w if norm else None, b if (norm and bias) else None, 1e-5, pos if rope else None,
                                 cos_t, sin_t)
    if dt == "bf16":
        tol = tol + R.half_ulp16(ref, False)
    _check(f"qk {path} {variant}", _np(got[:, :2]), ref, tol)
    if rope:     # the clamp is defined behaviour: positions -3 and npos + 5 give the bits of positions 0 and npos - 1
        assert tuple(pos[0]) == (-3, npos + 5)
        gb2, qkv2 = _guarded(DT[dt], (tokens, 3 * heads * 64), off)
        qkv2.copy_(src.reshape(tokens, -1))
        ops.qknorm_rope_(qkv2, heads, *wd, 1e-5, _at(np.clip(pos, 0, npos - 1), dtype=torch.int32), cos_d, sin_d)
        assert torch.equal(qkv, qkv2), "out-of-range positions must clamp to the table's ends"


@pytest.mark.parametrize("tokens,heads", R.QK_SHAPES)
@pytest.mark.parametrize("path", sorted(QK_PATHS))
def test_qknorm_rope(path, tokens, heads):
    for variant, npos in QK_PATHS[path][2]:
        _qk(path, tokens, heads, variant, npos)


def test_qknorm_rope_fast_grid_stride():
    """4100 x 16 head vectors: the grid caps at 2048 workgroups of 32, so the grid-stride loop makes a second, partial trip"""
    _qk("bf16 fast", 4100, 16, "norm+rope", 38)


# ------------------------------------------------------------------------------------------------------------------
# fp32 attention on strided streams
# ------------------------------------------------------------------------------------------------------------------
def _attn(key, bufs, offs, strides, *, batch, batch_inner, heads, seq_q, seq_k, hd, out_elems, unit=True, scale=None):
    """bufs: host float32 flat buffers (q, k, v) -- the same array may serve several streams; offs / strides per stream
    (q, k, v, out).  The output buffer of out_elems floats is NaN-prefilled and compared whole: rows the launch does not
    own must stay NaN, every row it owns must be written"""
    scale = 1.0 / np.sqrt(hd) if scale is None else scale
    dev = {}
    for a in bufs:
        if id(a) not in dev:
            dev[id(a)] = _at(a)
    q, k, v = (dev[id(a)].reshape(-1)[o:] for a, o in zip(bufs, offs))
    gb, out = _guarded(torch.float32, (out_elems,))
    dims = dict(batch=batch, batch_inner=batch_inner, heads=heads, hd=hd)
    qg, kg, vg = (R.gather_stream(a, o, s, seq=n, **dims) for a, o, s, n in zip(bufs, offs, strides, (seq_q, seq_k, seq_k)))
    ref, tol, err = R.attention_tol(qg, kg, vg, scale, unit)
    EMU_ERR[key] = max(EMU_ERR.get(key, 0.0), err)
    ops.attention_f32_strided(q, k, v, out[offs[3]:], q_strides=strides[0], k_strides=strides[1], v_strides=strides[2],
                              o_strides=strides[3], batch=batch, batch_inner=batch_inner, heads=heads, seq_q=seq_q, seq_k=seq_k,
                              head_dim=hd, scale=scale)
    plan = ops.attention_last_plan()   # the exact-fp32 kernel, HD 64 up to head_dim 64
    assert (plan.family, plan.hd, plan.grid) == (1, 64 if hd <= 64 else 128, -(-seq_q // 128) * heads * batch), plan
    _check_guards(gb)
    idx = R.stream_index(offs[3], strides[3], seq=seq_q, **dims).reshape(-1)
    assert len(np.unique(idx)) == idx.size, "the case's output rows overlap"
    want = np.full(out_elems, np.nan)
    want[idx] = ref.reshape(-1)
    got = _np(out)
    assert np.array_equal(np.isnan(got), np.isnan(want)), "an output element was left unwritten, or one outside the rows was written"
    _check(key, got[idx], want[idx], tol)


def _plain(key, q, k, v, unit=True, scale=None):
    """contiguous [B, H, seq, hd] streams in separate buffers"""
    B, H, sq, hd = q.shape
    sk = k.shape[2]
    st = lambda n: (hd, n * hd, H * n * hd, 0)      # noqa: E731
    _attn(key, (q.reshape(-1), k.reshape(-1), v.reshape(-1)), (0, 0, 0, 0), (st(sq), st(sk), st(sk), st(sq)), batch=B,
          batch_inner=0, heads=H, seq_q=sq, seq_k=sk, hd=hd, out_elems=q.size, unit=unit, scale=scale)


Hh, HEADS, HD48, B_, S_, V_, N_ = 96, 2, 48, 2, 3, 5, 37


def _randn(seed, *shape):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def test_attention_track_time():
    """run_mha's (vggt_track.hip) time attention: packed rows of 3 Hh, batch B (N + V), sequence S"""
    rows = B_ * (N_ + V_) * S_
    x = _randn(61, rows * 3 * Hh)
    s = (3 * Hh, HD48, S_ * 3 * Hh, 0)
    _attn("attn track time", (x, x, x), (0, Hh, 2 * Hh, 0), (s, s, s, (Hh, HD48, S_ * Hh, 0)), batch=B_ * (N_ + V_), batch_inner=0,
          heads=HEADS, seq_q=S_, seq_k=S_, hd=HD48, out_elems=rows * Hh)


def _cross(key, nq, nk, seed):
    """run_mha's space attention between two token sets: q on a [B][nq][S] stream of Hh, k / v on [B][nk][S] rows of 2 Hh;
    token stride S rows, inner batch (frame) stride one row, outer batch stride nq S / nk S rows"""
    q, kv = _randn(seed, B_ * nq * S_ * Hh), _randn(seed + 1, B_ * nk * S_ * 2 * Hh)
    sq, sk = (S_ * Hh, HD48, Hh, nq * S_ * Hh), (S_ * 2 * Hh, HD48, 2 * Hh, nk * S_ * 2 * Hh)
    _attn(key, (q, kv, kv), (0, 0, Hh, 0), (sq, sk, sk, sq), batch=B_ * S_, batch_inner=S_, heads=HEADS, seq_q=nq, seq_k=nk,
          hd=HD48, out_elems=B_ * nq * S_ * Hh)


def test_attention_track_v2p():
    _cross("attn track v2p", V_, N_, 62)


def test_attention_track_p2v():
    _cross("attn track p2v", N_, V_, 64)


def test_attention_track_virtual_self():
    """self attention over the V virtual tracks of a frame: packed 3 Hh rows on the transposed [B][V][S] layout"""
    x = _randn(66, B_ * V_ * S_ * 3 * Hh)
    s = (S_ * 3 * Hh, HD48, 3 * Hh, V_ * S_ * 3 * Hh)
    _attn("attn track virtual", (x, x, x), (0, Hh, 2 * Hh, 0), (s, s, s, (S_ * Hh, HD48, Hh, V_ * S_ * Hh)), batch=B_ * S_,
          batch_inner=S_, heads=HEADS, seq_q=V_, seq_k=V_, hd=HD48, out_elems=B_ * V_ * S_ * Hh)


@pytest.mark.parametrize("seq_q,seq_k", [(5, sk) for sk in (1, 31, 32, 33, 64, 65)] + [(sq, 40) for sq in (1, 32, 33, 127, 128, 129)])
def test_attention_sequence_edges(seq_q, seq_k):
    """seq_k on the 32-key tile edges, seq_q on the 128-query workgroup edges; one head, head_dim 64"""
    _plain("attn edges seq", _randn(70 + seq_q, 2, 1, seq_q, 64), _randn(71 + seq_k, 2, 1, seq_k, 64), _randn(72, 2, 1, seq_k, 64))


@pytest.mark.parametrize("hd", [4, 32, 36, 48, 64, 68, 100, 128])
def test_attention_head_dims(hd):
    """the kernel splits d over the lane halves at HD / 2 = 32 (head_dim <= 64) or 64"""
    _plain("attn edges head_dim", _randn(80 + hd, 1, 2, 37, hd), _randn(81 + hd, 1, 2, 37, hd), _randn(82 + hd, 1, 2, 37, hd))


@pytest.mark.parametrize("case", R.SOFTMAX_CASES)
def test_attention_softmax(case):
    q, k, v, unit = R.attention_softmax_case(case)
    _plain(f"attn softmax {case}", q, k, v, unit=unit, scale=0.125)


def test_attention_strided_argument_checks():
    """an error code and nothing launched: head_dim 0, 6, 132; a stride that is no multiple of 4; batch 70000"""
    x = _at(_randn(90, 4096))
    gb, out = _guarded(torch.float32, (4096,))
    ok = dict(q_strides=(64, 64, 0, 0), k_strides=(64, 64, 0, 0), v_strides=(64, 64, 0, 0), o_strides=(64, 64, 0, 0), batch=2,
              heads=1, seq_q=4, seq_k=4, head_dim=64)
    for bad, msg in ((dict(head_dim=0), "head_dim"), (dict(head_dim=6), "head_dim"), (dict(head_dim=132), "head_dim"),
                     (dict(k_strides=(66, 64, 0, 0)), "multiple of 4"), (dict(o_strides=(64, 64, 2, 0)), "multiple of 4"),
                     (dict(batch=70000), "grid dimension")):
        with pytest.raises(_lib.SkimiError, match=msg):
            ops.attention_f32_strided(x, x, x, out, **{**ok, **bad})
    with pytest.raises(_lib.SkimiError, match="past its buffer"):
        ops.attention_f32_strided(x, x, x, out, **{**ok, "seq_k": 80})
    torch.cuda.synchronize()
    gb.check()
    assert (gb.t == 0xFF).all()
