"""Thin torch-tensor wrappers over the generic C-ABI ops (skimi_gemm, skimi_layernorm,
skimi_qknorm_rope, skimi_attention).  Tensors provide device memory and the stream only; all
arithmetic happens in libskimi.so.  Used by the parity tests and by the Python host side."""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional

import torch

from . import _lib
from ._lib import ACT_NONE, BF16, F16, F32, PREC_BF16, PREC_BF16X3, GemmDesc, check, lib, ptr


def _dt(t: torch.Tensor) -> int:
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.bfloat16:
        return BF16
    if t.dtype == torch.float16:
        return F16
    raise TypeError(f"unsupported dtype {t.dtype}")


def _require_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise _lib.SkimiError("libskimi ops need device (HBM) tensors; got a CPU tensor")


def gemm(a, w, *, prec=PREC_BF16X3, bias=None, gamma=None, resid=None, act=ACT_NONE, out=None,
         out_dtype=torch.float32, conv=None, resid_map=None, pixel_shuffle=None, splitk_scratch=None,
         force_splitk=0, M=None, lda=None, w_split=None, x3_scratch=None, a_records=None, out_records=None,
         records_only=False, post_act=ACT_NONE, resid2=None, out2=None, out_map=None, splitk_zeroed=False):
    """out = epilogue(gather(a) @ w.T).  a: [rows, lda] (f32|bf16), w: [N, K].

    conv = dict(N,H,W,C,KH,KW,stride,pad,dil,OH,OW) selects the implicit-im2col gather;
    resid_map = (rows_per_batch, batch_stride, row_off); pixel_shuffle = (s, Cout, N, H, W).
    out_records = a `records_buffer(M, N)`: the result also as bf16x3 records (+ zero page) for a
    following `gemm(None, ..., a_records=that buffer)` (its [rows, C] shape comes through `conv`, or
    `M` and `lda` for plain rows); records_only: no fp32 result at all (returns None).
    post_act: activation applied after the residual adds.
    resid2: second residual, plain row m, the same dtype as resid; out2: the result again in the other
    dtype (bf16 next to an fp32 out, fp32 next to a 16-bit out), same indexing with its own row stride;
    out_map = (rows_per_batch, batch_stride, row_off): the output row remap (needs `out`: the rows it
    skips cannot be sized here); splitk_zeroed: the caller vouches that splitk_scratch is all zero (no memset)."""
    _require_cuda(w, bias, gamma, resid, out, resid2, out2)
    if out_map is not None and out is None:
        raise _lib.SkimiError("gemm: out_map needs a caller-owned out (the remapped rows cannot be sized here)")
    if resid is not None and resid2 is not None and resid.dtype != resid2.dtype:
        raise _lib.SkimiError("gemm: resid and resid2 share one dtype (resid_dtype)")
    d = GemmDesc()
    N, K = w.shape
    d.N, d.K = N, K
    d.W, d.w_dtype = ptr(w), _dt(w)
    if a_records is not None:
        _require_cuda(a_records)
        d.A, d.a_dtype = ptr(a_records), _lib.BF16X3_REC
        d.lda = lda if lda is not None else (conv["C"] if conv is not None else K)
    else:
        _require_cuda(a)
        d.A, d.a_dtype = ptr(a), _dt(a)
        d.lda = lda if lda is not None else a.stride(-2) if a.dim() >= 2 else a.shape[-1]
    dev = w.device
    d.ldw = w.stride(0)
    d.prec = prec
    if conv is not None:
        d.a_mode = 2 if conv.get("slice_major") else 1   # 2: weights packed [Cout][Cin/32][ky][kx][32]
        d.cN, d.cH, d.cW, d.cC = conv["N"], conv["H"], conv["W"], conv["C"]
        d.KH, d.KW, d.stride, d.pad, d.dil = conv["KH"], conv["KW"], conv["stride"], conv["pad"], conv["dil"]
        d.OH, d.OW = conv["OH"], conv["OW"]
        d.M = M if M is not None else d.cN * d.OH * d.OW   # an M of its own: only to test the library's refusal
    else:
        d.M = M if M is not None else a.shape[0]
    if records_only:
        assert out is None and out_records is not None and pixel_shuffle is None
        d.out_dtype = _lib.F32
    elif pixel_shuffle is not None:
        s, cout, n_img, h, w_ = pixel_shuffle
        d.store_mode, d.ps_s, d.ps_C = 1, s, cout
        d.cN, d.cH, d.cW = n_img, h, w_
        if out is None:
            out = torch.empty((n_img, h * s, w_ * s, cout), dtype=out_dtype, device=dev)
        d.ldo = out.stride(-2)
    else:
        if out is None:
            out = torch.empty((d.M, N), dtype=out_dtype, device=dev)
        d.ldo = out.stride(-2)
    if not records_only:
        d.out, d.out_dtype = ptr(out), _dt(out)
    if out2 is not None:
        if out is None or (out2.dtype == torch.float32) == (out.dtype == torch.float32) or \
                (out.dtype == torch.float32 and out2.dtype != torch.bfloat16):
            raise _lib.SkimiError("gemm: out2 is the other dtype of out (bf16 next to fp32, fp32 next to 16-bit)")
        d.out2, d.ldo2 = ptr(out2), out2.stride(-2)
    if out_map is not None:
        d.out_rows_per_batch, d.out_batch_stride, d.out_row_off = out_map
    d.bias, d.gamma, d.resid = ptr(bias), ptr(gamma), ptr(resid)
    if resid is not None:
        d.ldr = resid.stride(-2)
        d.resid_dtype = _dt(resid)
    if resid2 is not None:
        d.resid2, d.ldr2 = ptr(resid2), resid2.stride(-2)
        d.resid_dtype = _dt(resid2)
    if resid_map is not None:
        d.resid_rows_per_batch, d.resid_batch_stride, d.resid_row_off = resid_map
    d.act = act
    d.post_act = post_act
    if splitk_scratch is not None:
        d.splitk_scratch = ptr(splitk_scratch)
        d.splitk_scratch_bytes = splitk_scratch.numel() * splitk_scratch.element_size()
    d.force_splitk = force_splitk
    d.splitk_scratch_zeroed = int(splitk_zeroed)
    if w_split is not None:
        d.W_split = ptr(w_split)
        if a_records is not None:   # the zero page behind the records
            d.x3_scratch = ptr(a_records) + a_records.numel() * 2 - 256
            d.x3_scratch_bytes = 256
        else:
            d.x3_scratch = ptr(x3_scratch)
            d.x3_scratch_bytes = x3_scratch.numel() * x3_scratch.element_size()
    if out_records is not None:
        _require_cuda(out_records)
        d.out_records = ptr(out_records)
    check(lib().skimi_gemm(C.byref(d), _lib.current_stream()), "skimi_gemm")
    return out


class GemmPath(NamedTuple):
    """skimi_gemm_last_path decoded (field layout in include/skimi.h)"""
    family: Optional[str]   # generic | splitk_ordered | splitk_atomic | x3dma_wide | x3dma_narrow | gemm256 | conv_win
    tile: Optional[str]     # generic kernel: 64x64 | 128x64 | 128x128
    loop: Optional[str]     # gemm256: two_phase_256 | two_phase_192 | ping_pong | single_stream
    mfma: Optional[int]     # gemm256, x3dma: 16 (v_mfma_f32_16x16x32) | 32 (v_mfma_f32_32x32x16)
    epi: int                # gemm256: compile-time epilogue 0..3
    splitk: int             # K splits (1 = none)
    raw: int


_PATH_FAMILY = {1: "generic", 2: "splitk_ordered", 3: "splitk_atomic", 4: "x3dma_wide", 5: "x3dma_narrow",
                6: "gemm256", 7: "conv_win"}
_PATH_TILE = {1: "64x64", 2: "128x64", 3: "128x128"}
_PATH_LOOP = {1: "two_phase_256", 2: "two_phase_192", 3: "ping_pong", 4: "single_stream"}


def gemm_last_path() -> GemmPath:
    """which kernel the calling thread's last skimi_gemm dispatched to"""
    v = int(lib().skimi_gemm_last_path())
    fam = _PATH_FAMILY.get(v & 15)
    sub = (v >> 4) & 15
    generic = fam in ("generic", "splitk_ordered", "splitk_atomic")
    return GemmPath(family=fam, tile=_PATH_TILE.get(sub) if generic else None,
                    loop=_PATH_LOOP.get(sub) if fam == "gemm256" else None,
                    mfma={1: 16, 2: 32}.get((v >> 8) & 15), epi=(v >> 12) & 15, splitk=(v >> 16) & 255, raw=v)


def layernorm(x, gamma=None, beta=None, eps=1e-5, *, x2=None, out_dtype=torch.float32, out=None, rows=None, ldo=None,
              grp_rows=0, grp_stride=0, grp_off=0):
    """LayerNorm over the last dim of x (with x2: of the concatenation [x | x2], x2 on x's row stride).

    The keyword arguments after out_dtype make the launches of the forward (skimi_layernorm_ex); x is [in_rows, C] then,
    on any row stride.  grp_rows / grp_stride / grp_off: output row r reads input row (r // grp_rows) * grp_stride +
    grp_off + r % grp_rows; rows: output rows (default: every input row, or every whole group of the gather);
    out_dtype="records": bf16x3 records + zero page (a `records_buffer`); out: the destination -- for records any buffer of
    rows * C * 4 + 256 bytes, 128-byte aligned, else [rows, >= C] whose row stride is ldo (ldo= overrides it)."""
    _require_cuda(x, x2, gamma, beta, out)
    Cc = x.shape[-1] * (2 if x2 is not None else 1)
    if out is None and rows is None and ldo is None and not grp_rows and not isinstance(out_dtype, str):
        rows = x.numel() // x.shape[-1]
        out = torch.empty((*x.shape[:-1], Cc), dtype=out_dtype, device=x.device)
        check(lib().skimi_layernorm(ptr(x), ptr(x2), x.stride(-2), rows, Cc, ptr(gamma), ptr(beta), eps, ptr(out),
                                    _dt(out), Cc, _lib.current_stream()), "skimi_layernorm")
        return out
    if x.dim() != 2 or x.stride(-1) != 1 or (x2 is not None and (x2.shape != x.shape or x2.stride() != x.stride())):
        raise _lib.SkimiError("layernorm: the strided form takes x [in_rows, C] with unit column stride, x2 laid out like x")
    in_rows = x.shape[0]
    if rows is None:
        rows = in_rows // grp_stride * grp_rows if grp_rows else in_rows
    records = isinstance(out_dtype, str)
    if records:
        assert out_dtype == "records", out_dtype
        if out is None:
            out = records_buffer(rows, Cc, x.device)
        if out.numel() * out.element_size() < rows * Cc * 4 + 256:
            raise _lib.SkimiError("layernorm: `out` is too small for the records and their zero page")
        odt, ldo = _lib.BF16X3_REC, Cc
    else:
        if out is None:
            out = torch.empty((rows, ldo or Cc), dtype=out_dtype, device=x.device)
        odt = _dt(out)
        if out.dim() != 2 or out.stride(1) != 1 or out.shape[0] < rows or out.shape[1] < Cc:
            raise _lib.SkimiError("layernorm: `out` is [>= rows, >= C] with unit column stride")
        if ldo is None:
            ldo = out.stride(0)
        elif ldo != out.stride(0):
            raise _lib.SkimiError("layernorm: ldo is the row stride of `out`")
    check(lib().skimi_layernorm_ex(ptr(x), ptr(x2), x.stride(0), in_rows, rows, Cc, ptr(gamma), ptr(beta), eps, ptr(out), odt,
                                   ldo, grp_rows, grp_stride, grp_off, _lib.current_stream()), "skimi_layernorm_ex")
    return out


def qknorm_rope_(qkv, heads, qn_w=None, qn_b=None, kn_w=None, kn_b=None, eps=1e-5, pos=None, rope_cos=None,
                 rope_sin=None, *, q_scale=None):
    """in place on qkv [tokens, 3*heads*64].  q_scale: the block forward's call -- where the fast bf16 kernel runs, q is
    multiplied by q_scale before its one rounding to bf16; returns (qkv, q_scaled: bool) then"""
    _require_cuda(qkv, pos, rope_cos, rope_sin)
    tokens = qkv.numel() // (3 * heads * 64)
    npos = rope_cos.shape[0] if rope_cos is not None else 0
    if q_scale is not None:
        flag = C.c_int32(0)
        check(lib().skimi_qknorm_rope_scaled(ptr(qkv), _dt(qkv), tokens, heads, ptr(qn_w), ptr(qn_b), ptr(kn_w), ptr(kn_b),
                                             eps, ptr(pos), ptr(rope_cos), ptr(rope_sin), npos, q_scale, C.byref(flag),
                                             _lib.current_stream()), "skimi_qknorm_rope_scaled")
        return qkv, bool(flag.value)
    check(lib().skimi_qknorm_rope(ptr(qkv), _dt(qkv), tokens, heads, ptr(qn_w), ptr(qn_b), ptr(kn_w), ptr(kn_b),
                                  eps, ptr(pos), ptr(rope_cos), ptr(rope_sin), npos, _lib.current_stream()),
          "skimi_qknorm_rope")
    return qkv


def attention_x3_scratch_bytes(tokens, row_elems):
    """bytes of `x3_scratch` that selects the bf16x3 kernel for `tokens` packed fp32 qkv rows of `row_elems`"""
    return int(lib().skimi_attention_x3_scratch_bytes(tokens, row_elems))


class AttnPlan(NamedTuple):
    """skimi_attention_last_plan (include/skimi.h)"""
    family: int        # 0 none yet | 1 exact f32 | 2 bf16x3 | 3 bf16, 32 queries per wave | 4 bf16, 64 queries per wave
    queries: int       # per workgroup
    out_form: int      # 0 rows in the input type | 1 fp16 rows | 2 MXFP8 | 3 bf16x3 records
    q_prescaled: int   # as honoured
    grid: int          # workgroups
    hd: int            # the exact-f32 kernel's HD (64 elsewhere)
    lds: int           # bytes of dynamic LDS
    reserved: int


def attention_last_plan() -> AttnPlan:
    """the plan of the calling thread's last attention launch; a refused call leaves it as it was"""
    out = (C.c_int32 * 8)()
    lib().skimi_attention_last_plan(out)
    return AttnPlan(*out)


def attention(qkv, batch, seq, heads, head_dim, out_dtype=None, *, q_prescaled=0, x3_scratch=None, out_records=False,
              out=None):
    """qkv: [batch*seq, 3*heads*head_dim] -> [batch*seq, heads*head_dim] (same dtype; out_dtype=torch.float16 with
    bf16 qkv: the result rows as fp16, PREC_F16's proj operand; out_dtype="fp8mx" with bf16 qkv, head_dim 64: the result
    rows as MXFP8 -> (payload uint8 [rows, Kp], scales uint8 [rows, Kp/32]), PREC_FP8's proj operand)

    The keyword arguments make the block forward's launch (skimi_attention_ex): q_prescaled=1 for q that
    qknorm_rope_(q_scale=...) scaled; x3_scratch (a device tensor of >= attention_x3_scratch_bytes) selects the bf16x3
    kernel for fp32 qkv; out_records=True asks it for bf16x3 records in `out` (default: a `records_buffer`) and returns
    (out, written: bool) -- when not written, `out` holds the fp32 rows; out: the destination (any dtype, enough bytes)."""
    _require_cuda(qkv)
    if q_prescaled or x3_scratch is not None or out_records or out is not None:
        return _attention_ex(qkv, batch, seq, heads, head_dim, out_dtype, q_prescaled, x3_scratch, out_records, out)
    if isinstance(out_dtype, str):
        assert out_dtype == "fp8mx", out_dtype
        rows, Kp = batch * seq, (heads * head_dim + 127) // 128 * 128
        buf = torch.zeros(rows * (Kp + Kp // 32), dtype=torch.uint8, device=qkv.device)
        check(lib().skimi_attention_out(ptr(qkv), ptr(buf), _dt(qkv), _lib.FP8MX, batch, seq, heads, head_dim,
                                        _lib.current_stream()), "skimi_attention_out")
        return buf[:rows * Kp].view(rows, Kp), buf[rows * Kp:].view(rows, Kp // 32)
    out = torch.empty((batch * seq, heads * head_dim), dtype=out_dtype or qkv.dtype, device=qkv.device)
    if out_dtype is None or out_dtype == qkv.dtype:
        check(lib().skimi_attention(ptr(qkv), ptr(out), _dt(qkv), batch, seq, heads, head_dim, _lib.current_stream()),
              "skimi_attention")
    else:
        check(lib().skimi_attention_out(ptr(qkv), ptr(out), _dt(qkv), _dt(out), batch, seq, heads, head_dim,
                                        _lib.current_stream()), "skimi_attention_out")
    return out


def attention_f32_strided(q, k, v, out, *, q_strides, k_strides, v_strides, o_strides, batch, heads, seq_q, seq_k, head_dim,
                          scale=None, batch_inner=0):
    """The exact-fp32 attention kernel on four separate streams, as the track head launches it (skimi_attention_f32_strided).
    q / k / v / out: fp32 device tensors whose first element is the stream's origin (views into one buffer are fine);
    *_strides = (token, head, batch, outer batch) in elements; batch index g = go * batch_inner + gi (batch_inner = 0: one
    level).  scale defaults to 1 / sqrt(head_dim).  Every stream must fit the storage behind its tensor."""
    _require_cuda(q, k, v, out)
    no, ni = (batch // batch_inner, batch_inner) if batch_inner > 0 else (1, batch)
    for name, t, s, seq in (("q", q, q_strides, seq_q), ("k", k, k_strides, seq_k), ("v", v, v_strides, seq_k),
                            ("out", out, o_strides, seq_q)):
        if t.dtype != torch.float32:
            raise _lib.SkimiError(f"attention_f32_strided: {name} must be fp32")
        if len(s) != 4 or min(s) < 0:
            raise _lib.SkimiError(f"attention_f32_strided: {name}_strides = (token, head, batch, outer batch), not negative")
        room = t.untyped_storage().nbytes() // 4 - t.storage_offset()
        last = (seq - 1) * s[0] + (heads - 1) * s[1] + (ni - 1) * s[2] + (no - 1) * s[3] + head_dim
        if min(batch, heads, seq, head_dim) > 0 and last > room:
            raise _lib.SkimiError(f"attention_f32_strided: the {name} stream ends {last - room} elements past its buffer")
    arr = [(C.c_int64 * 4)(*map(int, s)) for s in (q_strides, k_strides, v_strides, o_strides)]
    sc = float(scale) if scale is not None else (1.0 / head_dim ** 0.5 if head_dim > 0 else 0.0)
    check(lib().skimi_attention_f32_strided(ptr(q), ptr(k), ptr(v), ptr(out), *arr, batch, batch_inner, heads, seq_q, seq_k,
                                            head_dim, sc, _lib.current_stream()), "skimi_attention_f32_strided")
    return out


def _attention_ex(qkv, batch, seq, heads, head_dim, out_dtype, q_prescaled, x3_scratch, out_records, out):
    _require_cuda(x3_scratch, out)
    rows, Cc = batch * seq, heads * head_dim
    flag = C.c_int32(1 if out_records else 0)
    sc_bytes = x3_scratch.numel() * x3_scratch.element_size() if x3_scratch is not None else 0
    mx = isinstance(out_dtype, str)
    if mx:
        assert out_dtype == "fp8mx", out_dtype
        odt, Kp = _lib.FP8MX, (Cc + 127) // 128 * 128
        need = rows * (Kp + Kp // 32)
        if out is None:
            out = torch.zeros(need, dtype=torch.uint8, device=qkv.device)
    else:
        odt = {torch.float32: F32, torch.bfloat16: BF16, torch.float16: F16}[out_dtype or qkv.dtype]
        need = rows * Cc * (4 if odt == F32 else 2) + (256 if out_records else 0)
        if out is None:
            out = records_buffer(rows, Cc, qkv.device) if out_records else \
                torch.empty((rows, Cc), dtype=out_dtype or qkv.dtype, device=qkv.device)
    assert out.numel() * out.element_size() >= need, "attention: `out` is too small"
    check(lib().skimi_attention_ex(ptr(qkv), ptr(out), _dt(qkv), odt, batch, seq, heads, head_dim, int(q_prescaled),
                                   ptr(x3_scratch), sc_bytes, C.byref(flag), _lib.current_stream()), "skimi_attention_ex")
    if mx:
        buf = out.view(torch.uint8).reshape(-1)
        return buf[:rows * Kp].view(rows, Kp), buf[rows * Kp:need].view(rows, Kp // 32)
    return (out, bool(flag.value)) if out_records else out


def conv3x3_n32_pack(w):
    """the reference's [32, C, 3, 3] fp32 weight -> the packed bf16 tensor [C/32, 2 (hi | lo), 9 (ky * 3 + kx), 32 (cout),
    32 (cin % 32)] that `conv3x3_n32(packed=...)` reads (skimi_conv3x3_n32_pack)"""
    _require_cuda(w)
    Cc = w.shape[1]
    assert w.shape == (32, Cc, 3, 3) and w.dtype == torch.float32
    packed = torch.empty(((Cc + 31) // 32, 2, 9, 32, 32), dtype=torch.bfloat16, device=w.device)
    check(lib().skimi_conv3x3_n32_pack(ptr(w.contiguous()), ptr(packed), Cc, _lib.current_stream()), "skimi_conv3x3_n32_pack")
    return packed


def conv3x3_n32(x, w, bias=None, relu=False, *, planes=None, px_stride=None, packed=None, out=None):
    """Direct fp32-accurate 3x3 conv (stride 1, pad 1) to 32 channels.  x: fp32 [F, H, W, C] channels-last,
    w: the reference's [32, C, 3, 3] fp32 weight -> fp32 [F, H, W, 32].

    The keyword arguments make the launches of the DPT heads (skimi_conv3x3_n32_strided); nothing is copied or checked
    here.  planes = (hi, lo): the bf16 planes of the input as they lie in memory (x is then its shape (F, H, W, C)), pixel
    p of a plane px_stride elements behind its first (default C; the heads' records [pixel][hi C | lo C]:
    planes = (rec, rec[C:]), px_stride = 2 C); packed: the weight from `conv3x3_n32_pack` (w is not read);
    out: the fp32 destination, F * H * W * 32 dense elements from its first."""
    _require_cuda(bias, packed, out)
    F_, H, W_, Cc = x if planes is not None else x.shape
    st = _lib.current_stream()
    if planes is None:
        _require_cuda(x)
        planes = split_planes(x.reshape(-1, Cc).contiguous())
        dev = x.device
    else:
        _require_cuda(*planes)
        dev = next((t.device for t in planes if t is not None), "cuda")
    if packed is None:
        assert w.shape == (32, Cc, 3, 3) and Cc % 32 == 0
        packed = conv3x3_n32_pack(w)
    if out is None:
        out = torch.empty((F_, H, W_, 32), dtype=torch.float32, device=dev)
    if px_stride is None:
        check(lib().skimi_conv3x3_n32(ptr(planes[0]), ptr(planes[1]), ptr(packed), ptr(bias), ptr(out), F_, H, W_, Cc,
                                      1 if relu else 0, st), "skimi_conv3x3_n32")
    else:
        check(lib().skimi_conv3x3_n32_strided(ptr(planes[0]), ptr(planes[1]), ptr(packed), ptr(bias), ptr(out), F_, H, W_,
                                              Cc, 1 if relu else 0, int(px_stride), st), "skimi_conv3x3_n32_strided")
    return out


def conv3x3_n32_upsampled(src, H, W, packed, bias=None, relu=False, *, tabx=None, taby=None, out=None):
    """A DPT head's tail (skimi_conv3x3_n32_upsampled): src [F, h, w, C] fp32 resized to H x W (align-corners bilinear, + the
    UV tables) and convolved 3x3 -> 32 by `conv3x3_n32`, in one launch where the shape allows -> (fp32 [F, H, W, 32], whether
    the one launch ran)"""
    _require_cuda(src, packed, bias, tabx, taby, out)
    F_, h, w, Cc = src.shape
    assert src.dtype == torch.float32 and src.is_contiguous()
    if out is None:
        out = torch.empty((F_, H, W, 32), dtype=torch.float32, device=src.device)
    rec = torch.empty((F_, H, W, 2 * Cc), dtype=torch.bfloat16, device=src.device)
    fused = C.c_int32(-1)
    check(lib().skimi_conv3x3_n32_upsampled(ptr(src), h, w, ptr(tabx), ptr(taby), ptr(packed), ptr(bias), ptr(out), F_, H, W, Cc,
                                            1 if relu else 0, ptr(rec), C.byref(fused), _lib.current_stream()),
          "skimi_conv3x3_n32_upsampled")
    return out, bool(fused.value)


def split_records(x):
    """fp32 [rows, C] -> bf16 [rows, ceil(C/32), 2, 32]: (hi, lo) halves of every 32-element slice in
    one 128-byte record (the `w_split` operand of `gemm`; a ragged last slice is zero-filled)."""
    _require_cuda(x)
    rows, Cc = x.shape
    out = torch.empty((rows, (Cc + 31) // 32, 2, 32), dtype=torch.bfloat16, device=x.device)
    check(lib().skimi_split_records(ptr(x), x.stride(0), rows, Cc, ptr(out), _lib.current_stream()), "skimi_split_records")
    return out


def records_buffer(rows, Cc, device="cuda"):
    """bf16 buffer for [rows, Cc] as bf16x3 records + the 256-byte zero page behind them."""
    return torch.empty(rows * ((Cc + 31) // 32) * 64 + 128, dtype=torch.bfloat16, device=device)


def x3_scratch_numel(rows, Cc):
    """fp32 elements of the `x3_scratch` that `gemm(..., w_split=...)` needs for an A buffer of [rows, Cc]."""
    return rows * ((Cc + 31) // 32 * 32) + 64


def dpt_fold_pack(w_T, b_T, w_rn):
    """ConvTranspose2d(kernel = stride = s) weight [Ci, Cm, s, s] (+ bias [Cm] or None) and the following bias-free 3x3
    conv's weight [Co, Cm, 3, 3] -> (weight records of the (s + 2)^2 phase taps, beta [9, Co]): the operands of
    `convT_conv3x3_folded` (skimi_dpt_fold_pack in include/skimi.h)."""
    _require_cuda(w_T, b_T, w_rn)
    Ci, Cm, s, s2 = w_T.shape
    Co = w_rn.shape[0]
    assert s == s2 and w_rn.shape == (Co, Cm, 3, 3)
    rec = torch.empty((s + 2) * (s + 2) * Co * Ci * 2, dtype=torch.bfloat16, device=w_T.device)
    beta = torch.empty((9, Co), dtype=torch.float32, device=w_T.device)
    check(lib().skimi_dpt_fold_pack(ptr(w_T.contiguous()), ptr(b_T.contiguous()) if b_T is not None else None, ptr(w_rn.contiguous()),
                                    Ci, Cm, Co, s, ptr(rec), ptr(beta), _lib.current_stream()), "skimi_dpt_fold_pack")
    return rec, beta


def convT_conv3x3_folded(x, w_records, beta, s, Co, *, act=ACT_NONE, out=None, out_records=None, records_only=False,
                         a_records=None):
    """conv2d(conv_transpose2d(x, w_T, b_T, stride = s), w_rn, padding = 1) of a channels-last fp32 x [F, h, w, Ci] in one
    launch of s x s phase convs on x (skimi_gemm_desc.a_mode 3; operands from `dpt_fold_pack`) -> fp32 [F, s h, s w, Co];
    out_records = a `records_buffer(F * s h * s w, Co)`: the result also (records_only: only) as bf16x3 records.
    a_records: x already as a `records_buffer(F * h * w, Ci)` (then x is its shape (F, h, w, Ci))."""
    _require_cuda(w_records, beta, out, out_records, a_records)
    F_, h, w_, Ci = x if a_records is not None else x.shape
    nrec = F_ * h * w_ * Ci * 2
    ar = a_records
    if ar is None:
        _require_cuda(x)
        ar = records_buffer(F_ * h * w_, Ci, device=x.device)
        ar[:nrec] = split_records(x.reshape(-1, Ci).contiguous()).reshape(-1)
        ar[nrec:] = 0
    d = GemmDesc()
    d.M, d.N, d.K = F_ * h * w_, Co, 4 * Ci
    d.A, d.a_dtype, d.lda = ptr(ar), _lib.BF16X3_REC, Ci
    d.W, d.w_dtype, d.ldw = ptr(w_records), _lib.F32, 4 * Ci
    d.W_split = ptr(w_records)
    d.x3_scratch, d.x3_scratch_bytes = ptr(ar) + nrec * 2, 256
    d.prec = PREC_BF16X3
    d.a_mode, d.store_mode, d.ps_s, d.ps_C = 3, 2, s, Co
    d.cN, d.cH, d.cW, d.cC = F_, h, w_, Ci
    d.bias, d.act = ptr(beta), act
    d.out_dtype = _lib.F32
    if not records_only:
        if out is None:
            out = torch.empty((F_, h * s, w_ * s, Co), dtype=torch.float32, device=w_records.device)
        d.out = ptr(out)
    d.ldo = Co
    if out_records is not None:
        d.out_records = ptr(out_records)
    check(lib().skimi_gemm(C.byref(d), _lib.current_stream()), "skimi_gemm")
    return out


def conv3x3_taps_matrix(w):
    """Conv2d weight [Co, Ci, 3, 3] -> the nine taps as stacked 1x1 matrices [9 Co, Ci] (row t Co + k = w[k, :, ty, tx],
    t = 3 ty + tx): the weight of the coarse-map contraction in front of `dpt_tap_sum` (Packer::conv_taps)."""
    Co, Ci = w.shape[:2]
    return w.permute(2, 3, 0, 1).reshape(9 * Co, Ci).contiguous()


def dpt_tap_sum(taps, bias, *, out=None):
    """taps [F, h, w, 9, C] fp32 (the nine tap contractions of a 3x3 / padding 1 conv on the coarse map) -> the conv of the
    x2 align-corners upsampled map, [F, 2h, 2w, C] fp32 (skimi_dpt_tap_sum in include/skimi.h)."""
    _require_cuda(taps, bias, out)
    F_, h, w_, nine, Cc = taps.shape
    assert nine == 9 and taps.is_contiguous() and taps.dtype == torch.float32
    if out is None:
        out = torch.empty((F_, 2 * h, 2 * w_, Cc), dtype=torch.float32, device=taps.device)
    check(lib().skimi_dpt_tap_sum(ptr(taps), ptr(bias), ptr(out), F_, h, w_, Cc, _lib.current_stream()), "skimi_dpt_tap_sum")
    return out


def split_planes(x):
    """fp32 [rows, C] -> bf16 [2, rows, C] (hi, lo) with hi + lo ~= x to ~2^-17 relative."""
    _require_cuda(x)
    rows, Cc = x.shape
    out = torch.empty((2, rows, Cc), dtype=torch.bfloat16, device=x.device)
    check(lib().skimi_split_planes(ptr(x), x.stride(0), rows, Cc, ptr(out[0]), ptr(out[1]), _lib.current_stream()),
          "skimi_split_planes")
    return out


def quant_mx(x: torch.Tensor):
    """x [rows, K] (f32 | bf16, device) -> (payload uint8 [rows, Kp], scales uint8 [rows, Kp / 32]): the MXFP8
    operand form of `gemm_fp8` (e4m3 elements, one E8M0 scale per 32 elements, Kp = K rounded up to 128)."""
    _require_cuda(x)
    x = x.contiguous()
    rows, K = x.shape
    Kp = (K + 127) // 128 * 128
    q = torch.empty((rows, Kp), dtype=torch.uint8, device=x.device)
    s = torch.empty((rows, Kp // 32), dtype=torch.uint8, device=x.device)
    check(lib().skimi_quant_mx(ptr(x), _dt(x), x.stride(0), rows, K, ptr(q), ptr(s), _lib.current_stream()), "skimi_quant_mx")
    return q, s


def layernorm_mx(x, gamma, beta, eps=1e-5):
    """LayerNorm of fp32 rows [rows, C] written directly as an MXFP8 operand (payload, scales) -- `quant_mx(layernorm(x))`
    in one pass (C % 256 == 0)."""
    _require_cuda(x, gamma, beta)
    rows, Cc = x.shape
    q = torch.empty((rows, Cc), dtype=torch.uint8, device=x.device)
    s = torch.empty((rows, Cc // 32), dtype=torch.uint8, device=x.device)
    check(lib().skimi_layernorm_mx(ptr(x), x.stride(0), rows, Cc, ptr(gamma), ptr(beta), eps, ptr(q), ptr(s),
                                   _lib.current_stream()), "skimi_layernorm_mx")
    return q, s


def gemm_fp8(a_q, a_s, w_q, w_s, K, *, bias=None, act=ACT_NONE, gamma=None, resid=None, out=None, out_dtype=torch.float32,
             out_mx=False):
    """out[m][n] = epilogue(sum_k A[m][k] W[n][k]) on the MXFP8 MFMA; operands from `quant_mx`.
    out_mx: return (payload uint8 [M, N], scales uint8 [M, N / 32]) -- the result directly as the next gemm_fp8's operand."""
    _require_cuda(a_q, a_s, w_q, w_s, bias, gamma, resid, out)
    M, N = a_q.shape[0], w_q.shape[0]
    Kp = (K + 127) // 128 * 128
    for t, cols, what in ((a_q, Kp, "a_q"), (w_q, Kp, "w_q"), (a_s, Kp // 32, "a_s"), (w_s, Kp // 32, "w_s")):
        if t.dtype != torch.uint8 or t.dim() != 2 or t.shape[1] != cols or not t.is_contiguous():
            raise _lib.SkimiError(f"gemm_fp8: {what} must be a contiguous uint8 [rows, {cols}] array for K = {K} "
                                  f"(got {tuple(t.shape)} {t.dtype}); operands come from quant_mx")
    if a_s.shape[0] != M or w_s.shape[0] != N:
        raise _lib.SkimiError("gemm_fp8: scale rows do not match the payload rows")
    if out_mx:
        q = torch.empty((M, N), dtype=torch.uint8, device=a_q.device)
        sc = torch.empty((M, N // 32), dtype=torch.uint8, device=a_q.device)
        check(lib().skimi_gemm_fp8(ptr(a_q), ptr(a_s), ptr(w_q), ptr(w_s), M, N, K, ptr(bias), act, None, None, 0, ptr(q),
                                   _lib.FP8MX, N, ptr(sc), _lib.current_stream()), "skimi_gemm_fp8")
        return q, sc
    if out is None:
        out = torch.empty((M, N), dtype=out_dtype, device=a_q.device)
    check(lib().skimi_gemm_fp8(ptr(a_q), ptr(a_s), ptr(w_q), ptr(w_s), M, N, K, ptr(bias), act, ptr(gamma), ptr(resid),
                               resid.stride(0) if resid is not None else 0, ptr(out), _dt(out), out.stride(0), None,
                               _lib.current_stream()), "skimi_gemm_fp8")
    return out


# ---- VGGT head / track-head helper kernels (include/skimi.h: one launch each).  Shapes come from the tensors; `out`
# arguments may be views into larger buffers (offsets, leading dimensions); nothing is computed here. ----
def _stream():
    return _lib.current_stream()


def resize_bilinear(x, H, W, *, out=None, out_dtype=None, tabx=None, taby=None, ln_g=None, ln_b=None, ln_eps=0.0):
    """x [N, h, w, C] -> [N, H, W, C], align_corners=True (+ UV tables, + LayerNorm over C == 128)"""
    _require_cuda(x, out, tabx, taby, ln_g, ln_b)
    N, h, w, Cc = x.shape
    if out is None:
        out = torch.empty((N, H, W, Cc), dtype=out_dtype or x.dtype, device=x.device)
    check(lib().skimi_resize_bilinear(ptr(x), ptr(out), _dt(x), _dt(out), N, h, w, H, W, Cc, ptr(tabx), ptr(taby), ptr(ln_g),
                                      ptr(ln_b), ln_eps, _stream()), "skimi_resize_bilinear")
    return out


def resize_bilinear_planes(x, H, W, out, *, tabx=None, taby=None, records=False, zpage=None):
    """x [N, h, w, C] fp32 -> out (16-bit elements, N * H * W * 2C of them) as bf16 hi / lo planes or records"""
    _require_cuda(x, out, tabx, taby, zpage)
    N, h, w, Cc = x.shape
    check(lib().skimi_resize_bilinear_planes(ptr(x), ptr(out), N, h, w, H, W, Cc, ptr(tabx), ptr(taby), int(records),
                                             ptr(zpage), _stream()), "skimi_resize_bilinear_planes")
    return out


def add_uv_pos_(x, tabx, taby):
    """x [N, H, W, C] += UV embedding, in place"""
    _require_cuda(x, tabx, taby)
    N, H, W, Cc = x.shape
    check(lib().skimi_add_uv_pos(ptr(x), _dt(x), ptr(tabx), ptr(taby), N, H, W, Cc, _stream()), "skimi_add_uv_pos")
    return x


def add_uv_pos_records(x, rec, tabx=None, taby=None):
    """x [N, H, W, C] fp32 (+ UV embedding) -> rec: bf16x3 records followed by the 256-byte zero page"""
    _require_cuda(x, rec, tabx, taby)
    N, H, W, Cc = x.shape
    check(lib().skimi_add_uv_pos_records(ptr(x), ptr(tabx), ptr(taby), N, H, W, Cc, ptr(rec), _stream()),
          "skimi_add_uv_pos_records")
    return rec


def dpt_out(x, weight, bias, mode, *, pts=None, conf=None):
    """x [npix, 32], weight [n_out, 32] -> (pts [npix, n_out - 1], conf [npix]); mode 0 exp, 1 inv_log"""
    _require_cuda(x, weight, bias, pts, conf)
    npix, n_out = x.shape[0], weight.shape[0]
    if pts is None:
        pts = torch.empty((npix, n_out - 1), dtype=torch.float32, device=x.device)
    if conf is None:
        conf = torch.empty((npix,), dtype=torch.float32, device=x.device)
    check(lib().skimi_dpt_out(ptr(x), _dt(x), ptr(weight), ptr(bias), n_out, ptr(pts), ptr(conf), npix, mode, _stream()),
          "skimi_dpt_out")
    return pts, conf


def patch_gather(img, p, Kp, *, out=None, out_dtype=torch.float32):
    """img [F, 3, H, W] fp32 -> [F * (H/p) * (W/p), Kp] normalised patches"""
    _require_cuda(img, out)
    F, _, H, W = img.shape
    if out is None:
        out = torch.empty((F * (H // p) * (W // p), Kp), dtype=out_dtype, device=img.device)
    check(lib().skimi_patch_gather(ptr(img), ptr(out), _dt(out), F, H, W, p, Kp, _stream()), "skimi_patch_gather")
    return out


def adaln(xn, x, mod, *, out=None):
    _require_cuda(xn, x, mod, out)
    rows, D = x.shape
    if out is None:
        out = torch.empty_like(x)
    check(lib().skimi_adaln(ptr(xn), ptr(x), ptr(mod), ptr(out), rows, D, _stream()), "skimi_adaln")
    return out


def pose_update_(delta, pred_pad, act_out, first):
    """pred_pad [rows, 16] updated in place from delta [rows, 9]; act_out [rows, 9]"""
    _require_cuda(delta, pred_pad, act_out)
    check(lib().skimi_pose_update(ptr(delta), ptr(pred_pad), ptr(act_out), delta.shape[0], int(first), _stream()),
          "skimi_pose_update")
    return act_out


def special_tokens_(x, table, S):
    """x [F, P, C]: rows 0..n-1 of every frame from table [2, n, C]"""
    _require_cuda(x, table)
    F, P, Cc = x.shape
    check(lib().skimi_special_tokens(ptr(x), ptr(table), F, S, P, table.shape[1], Cc, _stream()), "skimi_special_tokens")
    return x


def track_avgpool2(x, *, out=None):
    _require_cuda(x, out)
    N, H, W, Cc = x.shape
    if out is None:
        out = torch.empty((N, H // 2, W // 2, Cc), dtype=torch.float32, device=x.device)
    check(lib().skimi_track_avgpool2(ptr(x), ptr(out), N, H, W, Cc, _stream()), "skimi_track_avgpool2")
    return out


def track_sample_border(fmap, img_stride, coords, coord_stride, B, N, H, W, Cc, *, out=None):
    """fmap: B images [H, W, C] `img_stride` floats apart; coords: (x, y) every `coord_stride` floats -> [B, N, C]"""
    _require_cuda(fmap, coords, out)
    if out is None:
        out = torch.empty((B, N, Cc), dtype=torch.float32, device=fmap.device)
    check(lib().skimi_track_sample_border(ptr(fmap), img_stride, ptr(coords), coord_stride, ptr(out), B, N, H, W, Cc,
                                          _stream()), "skimi_track_sample_border")
    return out


def track_corr_sample(tgt, fmap, coords, out, N, S, r, level, ldo, out_off):
    """tgt [rows, C], fmap [B * S, H, W, C], coords [rows, 2] -> out[row * ldo + out_off + 0 .. (2r+1)^2 - 1]"""
    _require_cuda(tgt, fmap, coords, out)
    rows, Cc = tgt.shape
    _, H, W, _ = fmap.shape
    check(lib().skimi_track_corr_sample(ptr(tgt), ptr(fmap), ptr(coords), ptr(out), rows, N, S, H, W, Cc, r, level, ldo,
                                        out_off, _stream()), "skimi_track_corr_sample")
    return out


def track_pos_embed_sample(coords, coord_stride, BN, H, W, D, *, out=None):
    _require_cuda(coords, out)
    if out is None:
        out = torch.empty((BN, D), dtype=torch.float32, device=coords.device)
    check(lib().skimi_track_pos_embed_sample(ptr(coords), coord_stride, ptr(out), BN, H, W, D, _stream()),
          "skimi_track_pos_embed_sample")
    return out


def track_input(coords, fcorr, tfeat, pos, qrt, x, S, L, ldx, max_scale):
    """coords [rows, 2], fcorr / tfeat [rows, L], pos [rows / S, 3L + 4], qrt [2, 3L + 4] -> x, row stride ldx"""
    _require_cuda(coords, fcorr, tfeat, pos, qrt, x)
    check(lib().skimi_track_input(ptr(coords), ptr(fcorr), ptr(tfeat), ptr(pos), ptr(qrt), ptr(x), coords.shape[0], S, L, ldx,
                                  max_scale, _stream()), "skimi_track_input")
    return x


def track_coord_update_(coords, delta, ldd, query, N, S, stride, *, pred=None):
    """coords [rows, 2] += delta[:, :2] in place, rows s == 0 reset to query [rows / S, 2]; pred [B, S, N, 2] or None"""
    _require_cuda(coords, delta, query, pred)
    check(lib().skimi_track_coord_update(ptr(coords), ptr(delta), ldd, ptr(query), ptr(pred), coords.shape[0], N, S, stride,
                                         _stream()), "skimi_track_coord_update")
    return coords


def track_init(q, coords, qs, S, stride):
    """q [BN, 2] -> coords [BN, S, 2], qs [BN, 2], both q / stride"""
    _require_cuda(q, coords, qs)
    check(lib().skimi_track_init(ptr(q), ptr(coords), ptr(qs), q.shape[0], S, stride, _stream()), "skimi_track_init")
    return coords, qs


def track_repeat_rows(src, S, *, out=None):
    _require_cuda(src, out)
    BN, Cc = src.shape
    if out is None:
        out = torch.empty((BN, S, Cc), dtype=torch.float32, device=src.device)
    check(lib().skimi_track_repeat_rows(ptr(src), ptr(out), BN, S, Cc, _stream()), "skimi_track_repeat_rows")
    return out


def track_bns_to_bsn(x, *, out=None):
    _require_cuda(x, out)
    B, N, S = x.shape
    if out is None:
        out = torch.empty((B, S, N), dtype=torch.float32, device=x.device)
    check(lib().skimi_track_bns_to_bsn(ptr(x), ptr(out), B, N, S, _stream()), "skimi_track_bns_to_bsn")
    return out
