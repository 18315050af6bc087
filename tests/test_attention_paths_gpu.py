"""GPU: attention as the VGGT block forward launches it (vggt_block.hip: skimi_qknorm_rope_scaled + skimi_attention_ex),
not only as skimi_attention does -- the parity mode's bf16x3 kernel (hi + lo operands, three MFMAs per product) with
its scratch rule and its bf16x3 record output, and the prescaled-q chain of the bf16 / fp16 / fp8 modes (qk-norm folds
1/sqrt(64) * log2(e) into q before q's one rounding, the attention kernel then skips its own scale fold).

Every reference is float64 SDPA, softmax(q k^T / 8) v, on the CPU, from the exact values the kernel read (the bf16
q / k / v it loaded; for prescaled q the q that qk-norm stored, divided back by q_scale).  At long sequences the
reference covers a fixed, seeded sample of query rows (the first, the last and the whole last query block included)
against all keys."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import mxfp8_oracle as mx
from skiing_analysis_pytorch_amd import ops
from skiing_analysis_pytorch_amd._lib import PREC_BF16X3, SkimiError

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = Path(__file__).resolve().parent.parent
# the forward's q_scale, as the fp32 it passes: (1 / sqrtf(64)) * log2(e)
Q_SCALE = float(np.float32(0.125) * np.float32(1.44269504088896340736))

# ---------------------------------------------------------------------------------------------------------------------
# float64 reference
# ---------------------------------------------------------------------------------------------------------------------


def _rows(seq, n=512):
    """query rows the reference covers: all of them up to n, else a seeded sample plus the first, the last and the
    last 64 (the last wave of the 64-query kernel, two of the 32-query kernels)"""
    if seq <= n:
        return torch.arange(seq)
    g = torch.Generator().manual_seed(seq)
    fixed = torch.cat([torch.tensor([0, seq - 1]), torch.arange(seq - 64, seq)])
    return torch.unique(torch.cat([fixed, torch.randperm(seq, generator=g)[:n]]))


def _split(qkv, batch, seq, heads, hd=64):
    """packed [batch*seq, 3*heads*hd] (device) -> float64 q, k, v [batch, heads, seq, hd] (CPU)"""
    x = qkv.double().cpu().view(batch, seq, 3, heads, hd).permute(2, 0, 3, 1, 4)
    return x[0], x[1], x[2]


def _sdpa64(q, k, v, rows, spread=False):
    """float64 softmax(q[rows] k^T / sqrt(head_dim)) v -> [batch, heads, len(rows), head_dim] (head_dim 64: / 8);
    spread=True: also the largest sqrt(sum_j p_j^2) of a row (1 for a row on one key, ~1/sqrt(seq) for a flat one)"""
    B, H, S, hd = k.shape
    out = torch.empty(B, H, len(rows), hd, dtype=torch.float64)
    hc = max(1, min(H, (1 << 25) // (len(rows) * S)))   # heads per step: <= 256 MB of scores
    sp = 0.0
    for b in range(B):
        for h in range(0, H, hc):
            p = torch.softmax(q[b, h:h + hc, rows] @ k[b, h:h + hc].transpose(-1, -2) / float(hd) ** 0.5, -1)
            out[b, h:h + hc] = p @ v[b, h:h + hc]
            if spread:
                sp = max(sp, p.square().sum(-1).sqrt().max().item())
    return (out, sp) if spread else out


def _pick(out, batch, seq, heads, rows, hd=64):
    """kernel output [batch*seq, heads*hd] (device) -> float64 [batch, heads, len(rows), hd] (CPU)"""
    return out.double().cpu().view(batch, seq, heads, hd).permute(0, 2, 1, 3)[:, :, rows]


def _err(out, ref, batch, seq, heads, rows, hd=64):
    return (_pick(out, batch, seq, heads, rows, hd) - ref).abs().max().item()


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------


def _spikes(seq):
    """(query, key, factor): keys in an interior tile, in the ragged last tile and at the very last key
    (the cases of test_ops_gpu.py::test_attention_bf16_reference_moves_late, placed relative to seq)"""
    sp = {(0, seq - 1, 40.0), (seq - 1, seq // 2, 20.0), (seq // 3, max(seq - 3, 0), 16.0), (seq // 2, min(70, seq - 1), 24.0)}
    seen, out = set(), []
    for qi, ki, c in sorted(sp):
        if ki not in seen:
            seen.add(ki)
            out.append((qi, ki, c))
    return out


def _qkv(batch, seq, heads, case, seed):
    """float32 [batch*seq, 3*heads*64] on the CPU: randn; q x 4 (scores x 4); or the late-spike case -- q, k x 0.5 and
    chosen keys = a chosen query x c in every (batch, head)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(batch, seq, 3, heads, 64, generator=g)
    if case == "scores_x4":
        x[:, :, 0] *= 4.0
    elif case == "spikes":
        x[:, :, :2] *= 0.5
        for qi, ki, c in _spikes(seq):
            x[:, ki, 1] = x[:, qi, 0] * c
    return x.reshape(batch * seq, 3 * heads * 64)


# ---------------------------------------------------------------------------------------------------------------------
# a. the bf16x3 kernel (parity mode): fp32 in, fp32 out
# ---------------------------------------------------------------------------------------------------------------------

X3_SHAPES = [(1, 1, 1), (3, 63, 2), (1, 64, 1), (1, 65, 1), (2, 77, 3), (2, 257, 2), (8, 1374, 16), (1, 10992, 16)]
# Error model of the bf16x3 products: x = hi + lo, |lo| <= 2^-9 |x|, lo itself rounded with <= 2^-18 |x|; the kernel
# forms hi*hi + hi*lo + lo*hi, so one product of x and y is off by at most the dropped lo*lo (2^-18 |xy|) plus the two
# roundings of lo (2 * 2^-18 |xy|): about 2^-16.4 |xy|; the fp32 accumulation adds ~2^-24 per term.  A score (nats) is
# then off by up to 2^-16 * D, D = sum_i |q_i k_i| / 8 <= |q| |k| / 8, and softmax hands a score error on as a relative
# error of p_j, so o = sum_j p_j v_j moves by sum_j p_j (v_j - o) ds_j.  Stacked the same way, that is 2 * 2^-16 D max|v|;
# but the roundings are independent, so the sum grows like its root-sum-square: by sqrt(sum_j p_j^2), 1 for a row on
# one key, ~1/sqrt(seq) for a flat one (the splits of P and V add 3 * 2^-18 max|v|, the single-key case).  The unit:
#     u = 2^-16 * (1 + D) * max|v| * max_row sqrt(sum_j p_j^2)      (D from the largest |q| and |k| of a (batch, head))
# and the test asserts max |kernel - float64| <= X3_C * u.
#
# Measured on MI355X over the 24 shape x case runs below, in u: bf16x3 kernel 0.007 .. 0.031 (0.044 for seq 1: the
# splits of v alone); exact-fp32 kernel (SKIMI_ATTN_X3=0) <= 0.0093.  Max abs:
#   (8, 1374, 16):  bf16x3 3.9e-6 / 9.6e-5 / 1.5e-4 (randn / scores x 4 / spikes), fp32 1.1e-6 / 1.0e-5 / 1.3e-5
#   (1, 10992, 16): bf16x3 7.4e-7 / 9.1e-5 / 1.2e-4,                              fp32 3.7e-7 / 1.2e-5 / 5.0e-5
# X3_C = 0.12 is 2.7x the worst.  A kernel with only two of the three products (k's lo part dropped from QK^T, i.e. k
# rounded to bf16) is off by 3.0 .. 10.8 u on the same inputs (float64 emulation, asserted below to land > 16x outside).
X3_C = 0.12


def _x3_tol(q, k, v, spread):
    D = (q.norm(dim=-1).amax(-1) * k.norm(dim=-1).amax(-1) / float(q.shape[-1]) ** 0.5).max().item()
    return X3_C * 2.0 ** -16 * (1.0 + D) * v.abs().max().item() * spread, D


@pytest.mark.parametrize("case", ["randn", "scores_x4", "spikes"])
@pytest.mark.parametrize("batch,seq,heads", X3_SHAPES)
def test_attention_x3_fp32(batch, seq, heads, case, monkeypatch):
    """The bf16x3 kernel, selected the way the forward selects it (scratch of exactly skimi_attention_x3_scratch_bytes),
    and the exact-fp32 kernel on the same inputs, against float64 SDPA at the bound of the bf16x3 error model.  One byte
    less scratch falls back to the exact-fp32 kernel (bit for bit the scratch-less call), as does SKIMI_ATTN_X3=0."""
    tokens, C = batch * seq, heads * 64
    qkv = _qkv(batch, seq, heads, case, seed=1000 + seq).to(DEV)
    nb = ops.attention_x3_scratch_bytes(tokens, 3 * C)
    sc = torch.empty(nb, dtype=torch.uint8, device=DEV)
    fam = lambda: ops.attention_last_plan().family   # noqa: E731  (1 exact fp32, 2 bf16x3)
    x3 = ops.attention(qkv, batch, seq, heads, 64, x3_scratch=sc)
    assert fam() == 2
    less = ops.attention(qkv, batch, seq, heads, 64, x3_scratch=sc[:nb - 1])
    assert fam() == 1
    f32 = ops.attention(qkv, batch, seq, heads, 64)
    assert fam() == 1
    monkeypatch.setenv("SKIMI_ATTN_X3", "0")      # re-read per launch: conftest sets SKIMI_ENV_DYNAMIC=1
    f32_env = ops.attention(qkv, batch, seq, heads, 64, x3_scratch=sc)
    assert fam() == 1
    monkeypatch.delenv("SKIMI_ATTN_X3")
    assert torch.equal(less, f32) and torch.equal(f32_env, f32)
    if seq > 1:   # (one key: both kernels return v)
        assert not torch.equal(x3, f32), "the exact scratch size did not select the bf16x3 kernel"

    rows = _rows(seq)
    q, k, v = _split(qkv, batch, seq, heads)
    ref, spread = _sdpa64(q, k, v, rows, spread=True)
    tol, D = _x3_tol(q, k, v, spread)
    e_x3, e_f32 = _err(x3, ref, batch, seq, heads, rows), _err(f32, ref, batch, seq, heads, rows)
    unit = tol / X3_C
    print(f"\nMEASURED x3 {batch}x{seq}x{heads} {case}: x3 {e_x3:.3e} ({e_x3 / unit:.3f} u)  f32 {e_f32:.3e} "
          f"({e_f32 / unit:.3f} u)  bound {tol:.3e}  D {D:.1f}")
    assert torch.isfinite(x3).all()
    assert e_x3 <= tol, (e_x3, tol)
    assert e_f32 <= tol, (e_f32, tol)
    if seq > 1:
        # what a kernel that had lost one of the three products would be off by: k's lo part missing from QK^T
        two = _sdpa64(q, k.float().bfloat16().double(), v, rows)
        e_two = (two - ref).abs().max().item()
        print(f"MEASURED x3 {batch}x{seq}x{heads} {case}: two-product emulation {e_two:.3e} ({e_two / unit:.1f} u)")
        assert e_two > 16 * tol, (e_two, tol)


# ---------------------------------------------------------------------------------------------------------------------
# b. the bf16x3 kernel's record output (proj's operand in the parity mode)
# ---------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("batch,seq,heads", [(2, 300, 4), (1, 1374, 16), (3, 97, 8)])
def test_attention_x3_records(batch, seq, heads, monkeypatch):
    """out_records: [token][C/32][hi 32 | lo 32] bf16 records of the same fp32 quotient the kernel writes as rows (bit
    for bit the split of those rows), a 256-byte zero page behind them, and as the A operand of the proj GEMM the
    same result as the fp32 rows.  An `out` that is not 128-byte aligned gets fp32 rows and reports no records."""
    monkeypatch.setenv("SKIMI_X3_MIN_TILES", "1")   # let the small proj GEMM onto the LDS-DMA bf16x3 kernel
    tokens, C = batch * seq, heads * 64
    qkv = _qkv(batch, seq, heads, "randn", seed=2000 + seq).to(DEV)
    sc = torch.empty(ops.attention_x3_scratch_bytes(tokens, 3 * C), dtype=torch.uint8, device=DEV)
    rows32 = ops.attention(qkv, batch, seq, heads, 64, x3_scratch=sc)
    assert ops.attention_last_plan()[:3] == (2, 128, 0)   # bf16x3, fp32 rows

    rec = ops.records_buffer(tokens, C)
    rec.view(torch.uint8).fill_(0xFF)
    rec, written = ops.attention(qkv, batch, seq, heads, 64, x3_scratch=sc, out_records=True, out=rec)
    assert written
    assert ops.attention_last_plan()[:3] == (2, 128, 3)   # bf16x3, records
    r = rec[:tokens * C * 2].view(tokens, C // 32, 2, 32).float()
    hi, lo = r[:, :, 0].reshape(tokens, C), r[:, :, 1].reshape(tokens, C)
    # hi + lo reconstructs the fp32 quotient to 2^-18 relative (the issue's bar: 2^-16)
    assert ((hi + lo - rows32).abs() <= 2.0 ** -16 * rows32.abs()).all()
    assert torch.equal(rec[:tokens * C * 2].view(tokens, C // 32, 2, 32), ops.split_records(rows32))
    assert (rec.view(torch.uint8)[tokens * C * 4:] == 0).all()

    # proj: [C, C] weight + bias, records as A against the fp32 rows as A
    g = torch.Generator().manual_seed(C)
    w = (torch.randn(C, C, generator=g) / C ** 0.5).to(DEV)
    b = torch.randn(C, generator=g).to(DEV)
    ws = ops.split_records(w)
    y_rec = ops.gemm(None, w, prec=PREC_BF16X3, bias=b, a_records=rec, M=tokens, lda=C, w_split=ws)
    y_f32 = ops.gemm(rows32, w, prec=PREC_BF16X3, bias=b, w_split=ws,
                     x3_scratch=torch.empty(ops.x3_scratch_numel(tokens, C), dtype=torch.float32, device=DEV))
    ref = (rows32.double() @ w.double().T + b.double())
    rel = lambda a: ((a.double() - ref).norm() / ref.norm()).item()
    assert rel(y_rec) < 2e-5 and rel(y_f32) < 2e-5
    assert (y_rec - y_f32).abs().max().item() <= 1e-5 * ref.abs().max().item()

    # 64 bytes off the 128-byte alignment: fp32 rows, *out_records == 0
    big = torch.empty(tokens * C + 64 + 16, dtype=torch.float32, device=DEV)
    assert big.data_ptr() % 128 == 0
    out = big[16:]
    got, written = ops.attention(qkv, batch, seq, heads, 64, x3_scratch=sc, out_records=True, out=out)
    assert not written
    assert ops.attention_last_plan()[:3] == (2, 128, 0)
    assert torch.equal(got[:tokens * C].view(tokens, C), rows32)


# ---------------------------------------------------------------------------------------------------------------------
# c. the prescaled bf16 chain of the frame and global blocks
# ---------------------------------------------------------------------------------------------------------------------


def _rope_tables(npos, base=100.0):
    # vggt/vggt/layers/rope.py:86-117, fp32 (the tables the kernel reads)
    inv_freq = 1.0 / (base ** (torch.arange(0, 32, 2).float() / 32))
    ang = torch.einsum("i,j->ij", torch.arange(npos, dtype=torch.float32), inv_freq)
    return ang.cos().contiguous(), ang.sin().contiguous()


def _qknorm_rope_ref(t, w, b, pos, cos_t, sin_t):
    """float64 LayerNorm(64) + 2D RoPE of t [tokens, heads, 64] (rope.py:154-188: features 0..31 rotate by y, 32..63 by x,
    d pairs with d +- 16)"""
    t = torch.nn.functional.layer_norm(t, (64,), w.double(), b.double(), 1e-5)
    c2, s2 = torch.cat((cos_t, cos_t), -1).double(), torch.cat((sin_t, sin_t), -1).double()

    def one(x, p):
        rot = torch.cat((-x[..., 16:], x[..., :16]), -1)
        return x * c2[p][:, None] + rot * s2[p][:, None]

    return torch.cat((one(t[..., :32], pos[:, 0]), one(t[..., 32:], pos[:, 1])), -1)


def _chain_inputs(batch, seq, heads, case, npos=38):
    """bf16 qkv as qkv's epilogue leaves it, qk-norm weights and RoPE positions.  "spikes": qk-norm gammas of 2..3
    (checkpoint-sized scores: std ~ 9 nats between unrelated tokens) and the spiked keys copies of their query's raw
    vector at the same position, so that after norm and RoPE they are the query itself: a score of |q|^2 / 8 ~ 8 gamma^2"""
    g = torch.Generator().manual_seed(3000 + seq + heads)
    x = torch.randn(batch, seq, 3, heads, 64, generator=g)
    pos = torch.randint(0, npos, (batch, seq, 2), generator=g, dtype=torch.int32)
    if case == "spikes":
        gam = 2.0 + torch.rand(64, generator=g)
        qw, kw = gam, gam.clone()
        qb = kb = torch.zeros(64)
        for qi, ki, _ in _spikes(seq):
            x[:, ki, 1] = x[:, qi, 0]
            pos[:, ki] = pos[:, qi]
    else:
        qw, kw = 1.0 + 0.2 * torch.randn(64, generator=g), 1.0 + 0.2 * torch.randn(64, generator=g)
        qb, kb = 0.1 * torch.randn(64, generator=g), 0.1 * torch.randn(64, generator=g)
    qkv = x.reshape(batch * seq, 3 * heads * 64).to(torch.bfloat16)
    return qkv, (qw, qb, kw, kb), pos.reshape(batch * seq, 2)


def _half_ulp_bf16(x):
    _, e = torch.frexp(x)
    return torch.ldexp(torch.ones_like(x), e - 9)   # |x| in [2^(e-1), 2^e): bf16 ulp 2^(e-8)


def _half_ulp_f16(x):
    _, e = torch.frexp(x)
    return torch.ldexp(torch.ones_like(x), torch.clamp(e, min=-13) - 12)   # 11 significant bits; subnormal step 2^-24


def _assert_mx_rows(q8, s8, ref, batch, seq, rows):
    """MXFP8 output rows (payload, scales) against ref [batch, heads, len(rows), 64]: the bounds of
    test_fp8_gpu.py::test_attention_mx_output"""
    C = ref.shape[1] * 64
    sel = (torch.arange(batch)[:, None] * seq + rows[None]).reshape(-1)
    got = mx.mx_dequantize(q8.cpu().numpy()[sel][:, :C], s8.cpu().numpy()[sel][:, :C // 32])
    r = ref.permute(0, 2, 1, 3).reshape(-1, C).numpy()
    scale = np.exp2(s8.cpu().numpy()[sel][:, :C // 32].astype(np.float64) - 127.0).repeat(32, axis=1)
    tol = 2.0 ** -4 * np.abs(r) + scale * 2.0 ** -10 + 1.5e-2 * np.abs(r).max(axis=1, keepdims=True)
    assert (np.abs(got - r) <= tol).all(), float((np.abs(got - r) - tol).max())


CHAIN_SHAPES = [(3, 63, 2), (1, 65, 1), (2, 77, 4), (2, 257, 2), (1, 300, 6), (8, 1374, 16), (1, 10992, 16)]


@pytest.mark.parametrize("case", ["randn", "spikes"])
@pytest.mark.parametrize("batch,seq,heads", CHAIN_SHAPES)
def test_attention_prescaled_chain(batch, seq, heads, case):
    """qknorm_rope_(q_scale = log2(e) / 8) on bf16 qkv, then attention with q_prescaled=1 into bf16, fp16 (the f16 mode's
    proj operand) and MXFP8 rows (the fp8 mode's), as the frame and global blocks run it."""
    tokens, C = batch * seq, heads * 64
    qkv, (qw, qb, kw, kb), pos = _chain_inputs(batch, seq, heads, case)
    cos_t, sin_t = _rope_tables(38)
    dev = lambda t: t.to(DEV)
    args = (heads, dev(qw), dev(qb), dev(kw), dev(kb), 1e-5, dev(pos), dev(cos_t), dev(sin_t))
    buf, scaled = ops.qknorm_rope_(dev(qkv).clone(), *args, q_scale=Q_SCALE)
    assert scaled
    plain = ops.qknorm_rope_(dev(qkv).clone(), *args)

    # q as stored: bf16(normed q * q_scale), within half a bf16 ulp (+ the fp32 arithmetic of the kernel)
    x = qkv.double().view(tokens, 3, heads, 64)
    qn = _qknorm_rope_ref(x[:, 0], qw, qb, pos.long(), cos_t, sin_t) * Q_SCALE
    got_q = buf.double().cpu().view(tokens, 3, heads, 64)[:, 0]
    # (the kernel's fp32 norm + RoPE: a few fp32 ulps of the head's largest element)
    assert ((got_q - qn).abs() <= _half_ulp_bf16(qn) + 4e-6 * qn.abs().amax(-1, keepdim=True)).all()
    assert torch.equal(buf.view(tokens, 3, C)[:, 1:], plain.view(tokens, 3, C)[:, 1:])   # k and v as the unscaled call

    rows = _rows(seq)
    q, k, v = _split(buf, batch, seq, heads)
    ref = _sdpa64(q / Q_SCALE, k, v, rows)
    o_bf = ops.attention(buf, batch, seq, heads, 64, q_prescaled=1)
    o_16 = ops.attention(buf, batch, seq, heads, 64, out_dtype=torch.float16, q_prescaled=1)
    # the unprescaled path on the same normed q: the kernel folds the scale in itself, one more rounding of q to bf16
    qp, kp, vp = _split(plain, batch, seq, heads)
    q_eff = (qp.float() * Q_SCALE).bfloat16().double() / Q_SCALE
    o_pl = ops.attention(plain, batch, seq, heads, 64)
    ref_pl = _sdpa64(q_eff, kp, vp, rows)
    # per element: the output's own rounding (half an ulp of bf16 / fp16) + P rounded to bf16 in the PV product while
    # the row sum takes the fp32 p (<= 2^-9 max|v|, doubled).  For random data that stays inside test_attention_bf16's
    # 2e-2; rows that collapse onto one key (the spike cases) return |o| up to ~4.5, where half a bf16 ulp is 2^-7 .. 2^-6.
    slack = 2.0 ** -8 * v.abs().max().item()
    worst = {}
    for name, o, r, hu in (("bf16", o_bf, ref, _half_ulp_bf16), ("f16", o_16, ref, _half_ulp_f16),
                           ("unprescaled", o_pl, ref_pl, _half_ulp_bf16)):
        e = (_pick(o, batch, seq, heads, rows) - r).abs()
        worst[name] = (e.max().item(), (e - hu(r.abs() + slack) - slack).max().item())
    d_pl = (o_bf.float() - o_pl.float()).abs().max().item()
    print(f"\nMEASURED chain {batch}x{seq}x{heads} {case}: " +
          "  ".join(f"{n} {e:.3e} (bound margin {m:.1e})" for n, (e, m) in worst.items()) + f"  |prescaled - unprescaled| {d_pl:.3e}")
    for name, (e, m) in worst.items():
        assert m <= 0, (name, e, m)
        if case == "randn":
            assert e < 2e-2, (name, e)   # test_ops_gpu.py::test_attention_bf16
    if case == "randn":
        assert d_pl < 2e-2, d_pl

    if heads % 2 == 0:   # MXFP8 rows: the bounds of test_fp8_gpu.py::test_attention_mx_output
        q8, s8 = ops.attention(buf, batch, seq, heads, 64, out_dtype="fp8mx", q_prescaled=1)
        _assert_mx_rows(q8, s8, ref, batch, seq, rows)


# ---------------------------------------------------------------------------------------------------------------------
# d. the q_scaled flag: the non-fast qk-norm paths leave q unscaled and say so
# ---------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("path", ["fp32", "no_positions", "misaligned"])
def test_qknorm_q_scaled_flag(path):
    """Where qk-norm does not take the fast bf16 kernel (fp32 qkv; no RoPE positions; a qkv pointer that is not 16-byte
    aligned) it reports q_scaled == 0 and leaves q unscaled (the same bits as the call without q_scale), and attention
    with q_prescaled=0 on that buffer is right: the pairing the forward relies on."""
    batch, seq, heads = 2, 77, 2
    tokens, C = batch * seq, heads * 64
    qkv, (qw, qb, kw, kb), pos = _chain_inputs(batch, seq, heads, "randn")
    cos_t, sin_t = _rope_tables(38)
    dev = lambda t: t.to(DEV)
    if path == "fp32":
        qkv = qkv.float()
    p = None if path == "no_positions" else dev(pos)

    def fresh():
        if path != "misaligned":
            return dev(qkv).clone()
        big = torch.empty(qkv.numel() + 8, dtype=qkv.dtype, device=DEV)
        assert big.data_ptr() % 16 == 0
        t = big[1:1 + qkv.numel()].view(tokens, 3 * C)   # 2 bytes off
        t.copy_(dev(qkv))
        return t

    args = (heads, dev(qw), dev(qb), dev(kw), dev(kb), 1e-5, p, dev(cos_t), dev(sin_t))
    buf, scaled = ops.qknorm_rope_(fresh(), *args, q_scale=Q_SCALE)
    assert not scaled
    assert torch.equal(buf, ops.qknorm_rope_(fresh(), *args))
    aligned = buf.clone()
    rows = _rows(seq)
    q, k, v = _split(aligned, batch, seq, heads)
    out = ops.attention(aligned, batch, seq, heads, 64, q_prescaled=0)
    err = _err(out, _sdpa64(q, k, v, rows), batch, seq, heads, rows)
    assert err < (2e-5 if path == "fp32" else 2e-2), err
    if path == "fp32":   # fp32 q / k / v have no prescaled form: the flag is ignored
        assert torch.equal(ops.attention(aligned, batch, seq, heads, 64, q_prescaled=1), out)


def test_attention_bf16_refuses_misaligned_qkv():
    """The bf16 kernels load q / k / v in 16-byte pieces (LDS-DMA): a packed buffer that is not 16-byte aligned is an
    argument error, not a launch."""
    big = torch.zeros(64 * 3 * 64 + 8, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(SkimiError, match="16-B"):
        ops.attention(big[1:1 + 64 * 3 * 64].view(64, 192), 1, 64, 1, 64)


# ---------------------------------------------------------------------------------------------------------------------
# e. the 32-query kernel on the prescaled path
# ---------------------------------------------------------------------------------------------------------------------

_CHILD = r"""
import sys, torch
sys.path.insert(0, "tests")
import test_attention_paths_gpu as t
from skiing_analysis_pytorch_amd import ops
worst = 0.0
for batch, seq, heads in [(2, 77, 3), (1, 1374, 4), (2, 256, 2)]:
    qkv, (qw, qb, kw, kb), pos = t._chain_inputs(batch, seq, heads, "randn")
    cos_t, sin_t = t._rope_tables(38)
    d = lambda x: x.cuda()
    buf, scaled = ops.qknorm_rope_(d(qkv).clone(), heads, d(qw), d(qb), d(kw), d(kb), 1e-5, d(pos), d(cos_t), d(sin_t),
                                   q_scale=t.Q_SCALE)
    assert scaled
    rows = t._rows(seq)
    q, k, v = t._split(buf, batch, seq, heads)
    ref = t._sdpa64(q / t.Q_SCALE, k, v, rows)
    for odt in (None, torch.float16):
        out = ops.attention(buf, batch, seq, heads, 64, out_dtype=odt, q_prescaled=1)
        # the 32-query kernel, 128 queries per workgroup, bf16 / fp16 rows, q_prescaled honoured
        assert ops.attention_last_plan()[:4] == (3, 128, 0 if odt is None else 1, 1), ops.attention_last_plan()
        worst = max(worst, t._err(out, ref, batch, seq, heads, rows))
print("WORST", worst)
"""


def test_attention_prescaled_32_query_kernel():
    """SKIMI_ATTN_Q64=0 (the 32-query kernel, read once per process: a child process) on the prescaled chain: the
    launcher runs it with scale = ln 2 so that its own fold, scale * log2(e), is 1.  bf16 and fp16 rows, one ragged shape."""
    env = dict(os.environ, SKIMI_ATTN_Q64="0")
    r = subprocess.run([sys.executable, "-c", _CHILD], env=env, cwd=str(ROOT), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    worst = float(r.stdout.strip().split("WORST")[-1])
    print(f"\nMEASURED 32-query prescaled: {worst:.3e}")
    assert worst < 2e-2, worst
