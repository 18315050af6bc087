"""No GPU: the bounds of test_rowops_gpu.py hold for float32 emulations of the kernels' arithmetic (rowops_restated.py) on
every input family the GPU tests use, mutants of the emulations break them, and the argument checks of
skimi_layernorm_ex / skimi_attention_f32_strided, reached with null device pointers so that nothing is launched.
The worst error / bound per key is printed (profiles/rowops_tests.md)."""
import ctypes as C

import numpy as np
import pytest

import rowops_restated as R
from skiing_analysis_pytorch_amd import _lib

U = R.U
RATIOS = {}
LN_SCALAR_C = [1, 2, 63, 64, 65, 128, 129, 130, 388, 512, 516, 768, 1088, 1280, 1792, 2047]
LN_VECTOR_C = [256, 512, 768, 1024, 1536, 2048]
ROWS = 37


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(RATIOS):
        print(f"worst error / bound  {k:40s} {RATIOS[k]:.3g}")


def _ratio(key, got, ref, tol):
    err = np.abs(np.asarray(got, np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(tol > 0, err / tol, np.where(err == 0, 0.0, np.inf))
    worst = float(np.nan_to_num(r, nan=np.inf).max())
    if key:
        RATIOS[key] = max(RATIOS.get(key, 0.0), worst)
    return worst


def _ln_case(C, family, seed=0):
    g = np.random.default_rng(100 + C)
    x = R.ln_family(family, ROWS, C, 11 * C + seed)
    gamma = (1.0 + 0.5 * g.standard_normal(C)).astype(np.float32)
    beta = g.standard_normal(C).astype(np.float32)
    ref, cen, rstd = R.layernorm_ref(x, gamma, beta, 1e-5)
    return x, gamma, beta, ref, R.layernorm_tol(x, cen, rstd, ref, gamma)


@pytest.mark.parametrize("family", R.LN_FAMILIES)
@pytest.mark.parametrize("kernel,C", [("scalar", c) for c in LN_SCALAR_C] + [("vector", c) for c in LN_VECTOR_C])
def test_layernorm_emulation_meets_bound(kernel, C, family):
    x, gamma, beta, ref, tol = _ln_case(C, family)
    worst = _ratio(f"layernorm {kernel} {family}", R.layernorm_emulate(x, gamma, beta, 1e-5, kernel), ref, tol)
    assert worst <= 1.0, worst
    # null gamma / beta: the same bound with |gamma| = 1
    r0, c0, s0 = R.layernorm_ref(x, None, None, 1e-5)
    assert _ratio(f"layernorm {kernel} {family}", R.layernorm_emulate(x, None, None, 1e-5, kernel), r0,
                  R.layernorm_tol(x, c0, s0, r0, None)) <= 1.0


@pytest.mark.parametrize("kernel,C", [("scalar", c) for c in LN_SCALAR_C if c >= 63] + [("vector", c) for c in LN_VECTOR_C])
def test_layernorm_one_pass_variance_breaks_bound(kernel, C):
    x, gamma, beta, ref, tol = _ln_case(C, "mean1e3")
    worst = _ratio(None, R.layernorm_emulate(x, gamma, beta, 1e-5, kernel, mutant="one_pass"), ref, tol)
    RATIOS[f"mutant one_pass {kernel}"] = min(RATIOS.get(f"mutant one_pass {kernel}", np.inf), worst)
    assert worst > 1.0, worst


@pytest.mark.parametrize("kernel,C", [("scalar", 130), ("scalar", 768), ("vector", 512), ("vector", 2048)])
@pytest.mark.parametrize("family", R.LN_FAMILIES)
def test_layernorm_concat(kernel, C, family):
    """halves from different seeds with different means; the count of one half as the divisor must break the bound"""
    xa, xb = R.ln_family(family, ROWS, C // 2, 5 * C), R.ln_family(family, ROWS, C // 2, 5 * C + 1) + np.float32(0.75)
    x = R.ln_input(xa, xb)
    ref, cen, rstd = R.layernorm_ref(x, None, None, 1e-5)
    tol = R.layernorm_tol(x, cen, rstd, ref, None)
    assert _ratio(f"layernorm {kernel} concat", R.layernorm_emulate(x, None, None, 1e-5, kernel), ref, tol) <= 1.0
    bad = _ratio(None, R.layernorm_emulate(x, None, None, 1e-5, kernel, mutant="half_count"), ref, tol)
    RATIOS["mutant half_count"] = min(RATIOS.get("mutant half_count", np.inf), bad)
    assert bad > 1.0, bad


def test_gather_rows():
    assert R.gather_rows(4).tolist() == [0, 1, 2, 3]
    assert R.gather_rows(14, 6, 11, 5).tolist() == [5, 6, 7, 8, 9, 10, 16, 17, 18, 19, 20, 21, 27, 28]


# ---- q/k-norm + RoPE ----------------------------------------------------------------------------------------------------
QK_SHAPES = R.QK_SHAPES
qk_case = R.qk_case
QK_VARIANTS = {"norm+rope": (True, True, True), "norm only": (True, True, False), "rope only": (False, False, True),
               "null bias": (True, False, True)}


@pytest.mark.parametrize("variant", sorted(QK_VARIANTS))
@pytest.mark.parametrize("kernel", ["vec", "wave"])
@pytest.mark.parametrize("tokens,heads", QK_SHAPES)
def test_qknorm_rope_emulation_meets_bound(tokens, heads, kernel, variant):
    norm, bias, rope = QK_VARIANTS[variant]
    for npos in (38, 384, 385):
        cos_t, sin_t = R.rope_tables(npos)
        t, w, b, pos = qk_case(tokens, heads, npos)
        args = (w if norm else None, b if (norm and bias) else None, 1e-5, pos if rope else None, cos_t, sin_t)
        ref, tol = R.qknorm_rope_ref(t, *args)
        assert _ratio(f"qknorm_rope {kernel} {variant}", R.qknorm_rope_emulate(t, *args, kernel=kernel), ref, tol) <= 1.0


@pytest.mark.parametrize("mutant", ["sign", "swap_yx", "partner8"])
@pytest.mark.parametrize("kernel", ["vec", "wave"])
def test_qknorm_rope_mutants_break_bound(kernel, mutant):
    cos_t, sin_t = R.rope_tables(38)
    for tokens, heads in QK_SHAPES:
        t, w, b, pos = qk_case(tokens, heads, 38)
        pos[0] = (5, 9)     # not the clamped pair: position 0 rotates by nothing
        ref, tol = R.qknorm_rope_ref(t, w, b, 1e-5, pos, cos_t, sin_t)
        bad = _ratio(None, R.qknorm_rope_emulate(t, w, b, 1e-5, pos, cos_t, sin_t, kernel=kernel, mutant=mutant), ref, tol)
        RATIOS[f"mutant rope {mutant}"] = min(RATIOS.get(f"mutant rope {mutant}", np.inf), bad)
        assert bad > 1.0, (tokens, heads, bad)


def test_rope_clamp_is_defined():
    cos_t, sin_t = R.rope_tables(38)
    t, w, b, _ = qk_case(2, 1, 38)
    t[1] = t[0]
    out = R.qknorm_rope_emulate(t, w, b, 1e-5, np.array([[-3, 43], [0, 37]], np.int32), cos_t, sin_t)
    assert np.array_equal(out[0], out[1])


# ---- fp32 attention -----------------------------------------------------------------------------------------------------
def _attn_inputs(seq_q, seq_k, hd, seed, lead=(2, 2)):
    g = np.random.default_rng(seed)
    return tuple(g.standard_normal(lead + (n, hd)).astype(np.float32) for n in (seq_q, seq_k, seq_k))


ATTN_EDGES = ([(5, sk, 64) for sk in (1, 31, 32, 33, 64, 65)] + [(sq, 40, 64) for sq in (1, 32, 33, 127, 128, 129)] +
              [(37, 37, hd) for hd in (4, 32, 36, 48, 64, 68, 100, 128)] + [(3, 3, 48), (5, 37, 48), (37, 5, 48)])


@pytest.mark.parametrize("seq_q,seq_k,hd", ATTN_EDGES)
def test_attention_emulation_error(seq_q, seq_k, hd):
    """16 x the emulation's error stays under the 2e-5 of the older tests on unit-variance inputs: the cap does not bind"""
    q, k, v = _attn_inputs(seq_q, seq_k, hd, 900 + seq_q + seq_k + hd, lead=(1, 1))
    _, tol, err = R.attention_tol(q, k, v, 1.0 / np.sqrt(hd))
    RATIOS["attention 16 x emulation error / 2e-5"] = max(RATIOS.get("attention 16 x emulation error / 2e-5", 0.0), 16 * err / 2e-5)
    assert 16 * err <= 2e-5 and tol >= 16 * U * np.abs(v).max()


@pytest.mark.parametrize("case", R.SOFTMAX_CASES)
def test_attention_softmax_cases(case):
    q, k, v, unit = R.attention_softmax_case(case)
    ref, tol, err = R.attention_tol(q, k, v, 0.125, unit)
    print(f"{case}: emulation error {err:.3e}, tolerance {tol:.3e}")
    assert not unit or 16 * err <= 2e-5
    if case.startswith("spike"):      # the spiked key holds nearly all of query 0's weight
        j = 38 if case == "spike_last_tile" else 1
        assert np.abs(ref[0, 0, 0] - v[0, 0, j]).max() < 1e-6


@pytest.mark.parametrize("case", ["spike_last_tile", "scores_x4", "plain"])
def test_attention_without_alpha_breaks_tolerance(case):
    q, k, v, unit = R.attention_softmax_case(case, seq_k=70)
    ref, tol, _ = R.attention_tol(q, k, v, 0.125, unit)
    bad = np.abs(R.attention_emulate(q, k, v, 0.125, mutant="no_alpha") - ref).max() / tol
    RATIOS["mutant no_alpha"] = min(RATIOS.get("mutant no_alpha", np.inf), bad)
    assert bad > 1.0, bad


@pytest.mark.parametrize("seq_k", [1, 31, 33, 65, 40])
def test_attention_mask_off_by_one_breaks_tolerance(seq_k):
    q, k, v = _attn_inputs(5, seq_k, 64, 950 + seq_k, lead=(1, 1))
    ref, tol, _ = R.attention_tol(q, k, v, 0.125)
    bad = np.abs(R.attention_emulate(q, k, v, 0.125, mutant="mask_off_by_one") - ref).max() / tol
    RATIOS["mutant mask_off_by_one"] = min(RATIOS.get("mutant mask_off_by_one", np.inf), bad)
    assert bad > 1.0, bad


def test_gather_stream_two_level_batch():
    """the track head's transposed layout: token stride S rows, inner batch stride one row, outer batch V S rows"""
    B, V, S, W = 2, 5, 3, 8
    buf = np.arange(B * V * S * W)
    got = R.gather_stream(buf, 0, (S * W, 4, W, V * S * W), B * S, S, 2, V, 4)
    want = buf.reshape(B, V, S, 2, 4).transpose(0, 2, 3, 1, 4).reshape(B * S, 2, V, 4)
    assert np.array_equal(got, want)


# ---- argument checks of the two test entry points: null device pointers, nothing is launched --------------------------
def _ln_ex(in_rows, rows, C, out_dtype=_lib.F32, ldo=None, grp=(0, 0, 0), ldx=None):
    return _lib.lib().skimi_layernorm_ex(None, None, C if ldx is None else ldx, in_rows, rows, C, None, None, 1e-5, None,
                                         out_dtype, C if ldo is None else ldo, *grp, None)


@pytest.mark.parametrize("kw,msg", [
    (dict(in_rows=33, rows=18, C=128, grp=(6, 11, 5)), "bad arguments"),            # valid gather: stops at the null buffers
    (dict(in_rows=32, rows=18, C=128, grp=(6, 11, 5)), "input row 32 is read"),     # last row read is 2 * 11 + 5 + 5
    (dict(in_rows=33, rows=19, C=128, grp=(6, 11, 5)), "input row 38 is read"),
    (dict(in_rows=40, rows=6, C=128, grp=(6, 10, 5)), "grp_stride >= grp_off"),
    (dict(in_rows=40, rows=6, C=128, grp=(6, 11, -1)), "grp_off >= 0"),
    (dict(in_rows=40, rows=6, C=128, grp=(-6, 11, 0)), "negative"),
    (dict(in_rows=5, rows=6, C=128), "input row 5 is read"),
    (dict(in_rows=0, rows=6, C=128), "positive"),
    (dict(in_rows=6, rows=6, C=128, ldo=127), "below C"),
    (dict(in_rows=6, rows=6, C=256, ldo=0, out_dtype=_lib.BF16X3_REC), "bad arguments"),   # records: ldo unused
])
def test_layernorm_ex_argument_checks(kw, msg):
    assert _ln_ex(**kw) != 0
    assert msg in _lib.lib().skimi_last_error().decode()


def _attn_strided(batch=2, batch_inner=0, heads=2, seq_q=3, seq_k=3, hd=48, strides=None):
    s = [(C.c_int64 * 4)(*x) for x in (strides or [(96, 48, 288, 0)] * 4)]
    return _lib.lib().skimi_attention_f32_strided(None, None, None, None, *s, batch, batch_inner, heads, seq_q, seq_k, hd,
                                                  0.125, None)


@pytest.mark.parametrize("kw,msg", [
    (dict(), "null buffer"),                                                          # valid shape: stops at the null buffers
    (dict(batch=70000), "grid dimensions"),
    (dict(heads=70000), "grid dimensions"),
    (dict(batch=6, batch_inner=4), "must divide"),
    (dict(batch_inner=-1), "must divide"),
    (dict(strides=[(96, 48, 288, 0), (98, 48, 288, 0), (96, 48, 288, 0), (96, 48, 288, 0)]), "multiple of 4"),
    (dict(strides=[(96, 48, 288, 0)] * 3 + [(96, 48, 290, 0)]), "multiple of 4"),
    (dict(strides=[(96, 48, 288, 2)] + [(96, 48, 288, 0)] * 3), "multiple of 4"),
])
def test_attention_f32_strided_argument_checks(kw, msg):
    assert _attn_strided(**kw) != 0
    assert msg in _lib.lib().skimi_last_error().decode()
