"""What the attention launch plans, pinned row by row: plan_attention (csrc/attention.hip) and the exact-fp32 launcher.

TABLE holds one request on each side of every decision of that planning -- input type, head_dim, the bf16x3 scratch
rule, SKIMI_ATTN_X3, the record output and its alignment, the output form, q_prescaled -- at the sequence lengths where
the launchers and kernels change behaviour (1; 63 / 64 / 65, the 64-key tile; 127 / 128 / 129, the 128-query workgroup;
255 / 256 / 257, the 256-query workgroup), batch 2 so that the batch stride is exercised.  Every row asserts the whole
ops.attention_last_plan() against tests/golden/attention_plan.json and the output against float64 SDPA (the helpers
and the tolerances of test_attention_paths_gpu.py: the bf16x3 error model for fp32 input, 2e-2 for bf16 / fp16 rows,
test_fp8_gpu.py's bound for MXFP8 rows).  REFUSALS asserts return code and message, and that a refused call leaves the
plan as it was.

The golden is never written by the tree under test: `python tests/test_attention_plan_gpu.py`, run at the commit one
compares against with that commit's library, prints it as JSON (entry names in messages normalised to
`skimi_attention:`).  SKIMI_ATTN_Q64 is read once per process, so the 32-query rows run in one child process.

Left out: the 2^31-workgroup limit (no small shape reaches it)."""
import json
import os
import re
import subprocess
import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
if __name__ == "__main__":
    sys.path.insert(0, str(ROOT))
    sys.path.insert(0, str(ROOT / "tests"))
    os.environ.setdefault("SKIMI_ENV_DYNAMIC", "1")   # as tests/conftest.py sets it

import test_attention_paths_gpu as P  # noqa: E402  (float64 SDPA, the tolerances)
from skiing_analysis_pytorch_amd import _lib, ops  # noqa: E402
from skiing_analysis_pytorch_amd._lib import BF16, F16, F32, FP8MX, lib, ptr  # noqa: E402

DEV = "cuda"
GOLDEN = ROOT / "tests" / "golden" / "attention_plan.json"
f32, bf16, f16 = torch.float32, torch.bfloat16, torch.float16
SWITCHES = ("SKIMI_ATTN_X3", "SKIMI_ATTN_MX", "SKIMI_ATTN_Q64", "SKIMI_ATTN_LDSPAD", "SKIMI_ATTN_ABL")
ERR_ARG = -1


def _row(dt, seq, heads=2, hd=64, batch=2, **kw):
    """kw: out (f16 | "fp8mx"), prescaled, scratch ("exact" | "less"), env, records ("aligned" | "offset")"""
    return dict(dt=dt, batch=batch, seq=seq, heads=heads, hd=hd, **kw)


TABLE = {}
# fp32 without scratch: the exact kernel, HD 64 up to head_dim 64, HD 128 above
for hd in (32, 48, 64, 128):
    TABLE[f"f32_hd{hd}"] = _row(f32, 129, hd=hd)
for seq in (1, 127, 128):
    TABLE[f"f32_seq{seq}"] = _row(f32, seq)
TABLE["f32_heads3"] = _row(f32, 65, heads=3)
# fp32, head_dim 64, with scratch: bf16x3 from exactly attention_x3_scratch_bytes on
for seq in (1, 63, 64, 65, 127, 128, 129):
    TABLE[f"x3_seq{seq}"] = _row(f32, seq, scratch="exact")
TABLE["x3_heads1"] = _row(f32, 65, heads=1, scratch="exact")
TABLE["x3_heads3"] = _row(f32, 65, heads=3, scratch="exact")
TABLE["x3_one_byte_less"] = _row(f32, 129, scratch="less")
TABLE["x3_switched_off"] = _row(f32, 129, scratch="exact", env={"SKIMI_ATTN_X3": "0"})
TABLE["x3_hd128"] = _row(f32, 129, hd=128, scratch="exact")
TABLE["x3_prescaled_ignored"] = _row(f32, 65, scratch="exact", prescaled=1)
# records: written by the bf16x3 kernel into a 128-byte aligned `out` only
TABLE["records_aligned"] = _row(f32, 129, scratch="exact", records="aligned")
TABLE["records_offset_64_bytes"] = _row(f32, 129, scratch="exact", records="offset")
TABLE["records_exact_f32"] = _row(f32, 129, records="aligned")
TABLE["records_x3_switched_off"] = _row(f32, 129, scratch="exact", records="aligned", env={"SKIMI_ATTN_X3": "0"})
# bf16: the 64-query kernel, 256 queries per workgroup
for seq in (1, 63, 64, 65, 255, 256, 257):
    TABLE[f"bf16_seq{seq}"] = _row(bf16, seq)
TABLE["bf16_heads1"] = _row(bf16, 257, heads=1)
TABLE["bf16_heads3"] = _row(bf16, 257, heads=3)
TABLE["bf16_f16_rows"] = _row(bf16, 257, out=f16)
TABLE["bf16_mx_rows"] = _row(bf16, 257, out="fp8mx")
TABLE["bf16_prescaled"] = _row(bf16, 257, prescaled=1)
TABLE["bf16_prescaled_f16_rows"] = _row(bf16, 65, prescaled=1, out=f16)
TABLE["bf16_prescaled_mx_rows"] = _row(bf16, 65, prescaled=1, out="fp8mx")
TABLE["f32_prescaled_ignored"] = _row(f32, 65, prescaled=1)

# SKIMI_ATTN_Q64=0 (child process): the 32-query kernel, 128 queries per workgroup
Q32 = {
    "q32_seq127": _row(bf16, 127),
    "q32_seq128": _row(bf16, 128),
    "q32_seq129": _row(bf16, 129),
    "q32_seq129_prescaled": _row(bf16, 129, prescaled=1),
    "q32_f16_rows": _row(bf16, 129, out=f16),
}
Q32_REFUSED = "q32_mx_refused"   # the MXFP8 request of bf16_mx_rows under SKIMI_ATTN_Q64=0

# skimi_attention_f32_strided on the packed buffer: one-level and two-level batch
STRIDED = {"strided_inner0": 0, "strided_inner2": 2}
STRIDED_SHAPE = dict(batch=2, seq=129, heads=2, hd=48)


def _inputs(r):
    """bf16 / fp32 packed qkv on the device (seeded); prescaled bf16 rows carry q * Q_SCALE before the rounding"""
    batch, seq, heads, hd = r["batch"], r["seq"], r["heads"], r["hd"]
    g = torch.Generator().manual_seed(7000 + seq + 17 * heads + hd)
    x = torch.randn(batch, seq, 3, heads, hd, generator=g)
    if r.get("prescaled") and r["dt"] == bf16:
        x[:, :, 0] *= P.Q_SCALE
    return x.reshape(batch * seq, 3 * heads * hd).to(r["dt"]).to(DEV)


def launch(r):
    """one ops.attention launch of row `r` -> (plan as a list, written or None, output, qkv)"""
    batch, seq, heads, hd = r["batch"], r["seq"], r["heads"], r["hd"]
    tokens, Cc = batch * seq, heads * hd
    qkv = _inputs(r)
    kw = {}
    if r.get("scratch"):
        nb = ops.attention_x3_scratch_bytes(tokens, 3 * Cc)
        kw["x3_scratch"] = torch.empty(nb, dtype=torch.uint8, device=DEV)[:nb - (r["scratch"] == "less")]
    if r.get("records"):
        big = torch.empty(tokens * Cc + 64 + 16, dtype=f32, device=DEV)
        assert big.data_ptr() % 128 == 0
        kw.update(out_records=True, out=big if r["records"] == "aligned" else big[16:])
    if r.get("prescaled"):
        kw["q_prescaled"] = 1
    env = r.get("env", {})
    for k, v in env.items():
        os.environ[k] = v   # re-read per launch under SKIMI_ENV_DYNAMIC=1
    try:
        out = ops.attention(qkv, batch, seq, heads, hd, r.get("out"), **kw)
    finally:
        for k in env:
            del os.environ[k]
    plan = list(ops.attention_last_plan())
    torch.cuda.synchronize()
    written = None
    if r.get("records"):
        out, written = out
    return plan, written, out, qkv


def check_numbers(r, written, out, qkv):
    """the output of row `r` against float64 SDPA of the values the kernel read"""
    batch, seq, heads, hd = r["batch"], r["seq"], r["heads"], r["hd"]
    rows = P._rows(seq)
    q, k, v = P._split(qkv, batch, seq, heads, hd)
    if r["dt"] == f32:   # the bound of test_attention_x3_fp32, for the bf16x3 and the exact kernel alike
        ref, spread = P._sdpa64(q, k, v, rows, spread=True)
        tol, _ = P._x3_tol(q, k, v, spread)
        if written:
            rec = out.view(-1)[:batch * seq * heads * hd].view(torch.int16).view(bf16)
            rec = rec.view(batch * seq, heads * hd // 32, 2, 32).float()
            out = (rec[:, :, 0] + rec[:, :, 1]).reshape(batch * seq, heads * hd)
            tol += 2.0 ** -16 * ref.abs().max().item()   # hi + lo: test_attention_x3_records' bar
        else:
            out = out.view(-1)[:batch * seq * heads * hd].view(batch * seq, heads * hd)
        err = P._err(out, ref, batch, seq, heads, rows, hd)
        assert err <= tol, (err, tol)
        return
    ref = P._sdpa64(q / P.Q_SCALE if r.get("prescaled") else q, k, v, rows)
    if r.get("out") == "fp8mx":
        P._assert_mx_rows(out[0], out[1], ref, batch, seq, rows)
        return
    assert out.dtype == (r.get("out") or bf16)
    err = P._err(out, ref, batch, seq, heads, rows)
    assert err < 2e-2, err   # test_attention_prescaled_chain / test_ops_gpu.py::test_attention_bf16, randn


def launch_strided(batch_inner):
    """the packed qkv of STRIDED_SHAPE through skimi_attention_f32_strided -> (plan, packed call's plan, out, packed out, qkv)"""
    r = _row(f32, **STRIDED_SHAPE)
    batch, seq, heads, hd = r["batch"], r["seq"], r["heads"], r["hd"]
    Cc = heads * hd
    qkv = _inputs(r)
    packed = ops.attention(qkv, batch, seq, heads, hd)
    packed_plan = list(ops.attention_last_plan())
    flat = qkv.view(-1)
    out = torch.empty(batch * seq * Cc, dtype=f32, device=DEV)
    outer = batch_inner * seq   # rows per outer batch step (one outer step when batch_inner == batch)
    s_in, s_out = (3 * Cc, hd, seq * 3 * Cc, outer * 3 * Cc), (Cc, hd, seq * Cc, outer * Cc)
    ops.attention_f32_strided(flat, flat[Cc:], flat[2 * Cc:], out, q_strides=s_in, k_strides=s_in, v_strides=s_in,
                              o_strides=s_out, batch=batch, heads=heads, seq_q=seq, seq_k=seq, head_dim=hd,
                              batch_inner=batch_inner)
    plan = list(ops.attention_last_plan())
    torch.cuda.synchronize()
    return r, plan, packed_plan, out.view(batch * seq, Cc), packed, qkv


def _call_ex(qkv, out, dt, odt, batch, seq, heads, hd):
    """skimi_attention_ex on raw addresses -> (return code, message with the entry's name normalised)"""
    rc = lib().skimi_attention_ex(qkv, out, dt, odt, batch, seq, heads, hd, 0, None, 0, None, _lib.current_stream())
    msg = lib().skimi_last_error().decode() if rc else ""
    return rc, re.sub(r"^skimi_attention(_out|_ex)?:", "skimi_attention:", msg)


def _refusals():
    """name -> a callable that makes the refused call on `buf` (a zeroed device buffer, 256-byte aligned)"""
    def ex(dt, odt, batch=2, seq=65, heads=2, hd=64, q_off=0, null_q=False, null_out=False):
        def go(buf):
            q = None if null_q else buf.data_ptr() + q_off
            o = None if null_out else buf.data_ptr() + (1 << 20)
            return _call_ex(q, o, dt, odt, batch, seq, heads, hd)
        return go

    return {
        "null_qkv": ex(BF16, BF16, null_q=True),
        "null_out": ex(F32, F32, null_out=True),
        "empty_batch_bf16": ex(BF16, BF16, batch=0),
        "empty_seq_f32": ex(F32, F32, seq=0),
        "bf16_hd32": ex(BF16, BF16, hd=32),
        "bf16_qkv_off_8_bytes": ex(BF16, BF16, q_off=8),
        "f32_hd132": ex(F32, F32, hd=132),
        "f32_hd30": ex(F32, F32, hd=30),
        "mx_heads1": ex(BF16, FP8MX, heads=1),
        "mx_heads3": ex(BF16, FP8MX, heads=3),
        "mx_f32_input": ex(F32, FP8MX),
        "bad_out_dtype_pair": ex(F32, BF16),
    }


# not in the golden: the commit it was recorded at read an fp16 buffer as bf16 and returned SKIMI_OK
NEW_REFUSALS = {"dtype_f16": (F16, F16, "skimi_attention: dtype must be SKIMI_F32 or SKIMI_BF16")}


def run_refusal(go):
    buf = torch.zeros(1 << 21, dtype=torch.uint8, device=DEV)
    ops.attention(torch.zeros(8, 3 * 64, dtype=bf16, device=DEV), 1, 8, 1, 64)   # a plan to be left alone
    before = list(ops.attention_last_plan())
    rc, msg = go(buf)
    after = list(ops.attention_last_plan())
    torch.cuda.synchronize()
    return dict(code=rc, message=msg), before, after


def run_q32_rows():
    """the Q32 rows and the refused MXFP8 request, in this process (SKIMI_ATTN_Q64=0 set by the parent process)"""
    assert os.environ.get("SKIMI_ATTN_Q64") == "0"
    got = {}
    for name, r in Q32.items():
        plan, written, out, qkv = launch(r)
        check_numbers(r, written, out, qkv)
        got[name] = dict(plan=plan, written=written)
    r = TABLE["bf16_mx_rows"]
    qkv, buf = _inputs(r), torch.zeros(1 << 21, dtype=torch.uint8, device=DEV)
    before = list(ops.attention_last_plan())
    rc, msg = _call_ex(qkv.data_ptr(), buf.data_ptr(), BF16, FP8MX, r["batch"], r["seq"], r["heads"], r["hd"])
    assert list(ops.attention_last_plan()) == before, "a refused call moved the plan"
    got[Q32_REFUSED] = dict(code=rc, message=msg)
    return got


def run_q32_child():
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env["SKIMI_ATTN_Q64"] = "0"
    p = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--q32-rows"], env=env, cwd=str(ROOT),
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


gpu = pytest.mark.gpu


def _golden():
    return json.loads(GOLDEN.read_text())


def test_table_and_golden_have_the_same_rows():
    assert sorted(_golden()) == sorted([*TABLE, *Q32, Q32_REFUSED, *STRIDED, *_refusals()])


@gpu
@pytest.mark.parametrize("name", list(TABLE))
def test_plan_table(monkeypatch, name):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    r, want = TABLE[name], _golden()[name]
    plan, written, out, qkv = launch(r)
    assert plan == want["plan"], f"{name}: planned {plan}, recorded {want['plan']}"
    assert written == want["written"]
    check_numbers(r, written, out, qkv)


def test_plan_table_decisions():
    """the golden itself says what the issue of this table asks of each side of a decision"""
    g = _golden()
    fam = lambda n: g[n]["plan"][0]        # noqa: E731
    form = lambda n: g[n]["plan"][2]       # noqa: E731
    assert [g[f"f32_hd{hd}"]["plan"][5] for hd in (32, 48, 64, 128)] == [64, 64, 64, 128]
    assert all(fam(n) == 1 for n in ("f32_hd64", "x3_one_byte_less", "x3_switched_off", "x3_hd128", "records_exact_f32"))
    assert fam("x3_seq129") == 2 and form("x3_seq129") == 0
    assert (form("records_aligned"), g["records_aligned"]["written"]) == (3, True)
    assert (form("records_offset_64_bytes"), g["records_offset_64_bytes"]["written"]) == (0, False)
    assert g["records_exact_f32"]["written"] is False and g["records_x3_switched_off"]["written"] is False
    for seq in (1, 63, 64, 65, 255, 256, 257):
        assert g[f"bf16_seq{seq}"]["plan"] == [4, 256, 0, 0, -(-seq // 256) * 2 * 2, 64, 0, 0]
    assert form("bf16_f16_rows") == 1 and form("bf16_mx_rows") == 2
    assert g["bf16_prescaled"]["plan"][3] == 1 and g["f32_prescaled_ignored"]["plan"][3] == 0
    assert g["x3_prescaled_ignored"]["plan"][3] == 0
    assert g["q32_seq129"]["plan"] == [3, 128, 0, 0, 2 * 2 * 2, 64, 0, 0]
    assert g["q32_seq129_prescaled"]["plan"] == [3, 128, 0, 1, 2 * 2 * 2, 64, 0, 0]


@gpu
def test_plan_table_32_query_kernel():
    got, want = run_q32_child(), _golden()
    assert sorted(got) == sorted([*Q32, Q32_REFUSED])
    for name in got:
        assert got[name] == want[name], (name, got[name], want[name])
    assert want[Q32_REFUSED]["code"] == ERR_ARG and "MXFP8 rows need bf16" in want[Q32_REFUSED]["message"]


@gpu
@pytest.mark.parametrize("name", list(STRIDED))
def test_plan_strided(name):
    r, plan, packed_plan, out, packed, qkv = launch_strided(STRIDED[name])
    assert plan == _golden()[name]["plan"], (plan, _golden()[name]["plan"])
    assert plan[0] == 1 and plan[4] == packed_plan[4]
    assert torch.equal(out, packed)
    check_numbers(r, None, out, qkv)


@gpu
@pytest.mark.parametrize("name", list(_refusals()))
def test_plan_refusals(name):
    got, before, after = run_refusal(_refusals()[name])
    want = _golden()[name]
    assert got["code"] == want["code"] == ERR_ARG
    assert got["message"] == want["message"], (got["message"], want["message"])
    assert after == before, "a refused call moved the plan"


@gpu
@pytest.mark.parametrize("name", list(NEW_REFUSALS))
def test_plan_new_refusals(name):
    dt, odt, message = NEW_REFUSALS[name]
    got, before, after = run_refusal(lambda buf: _call_ex(buf.data_ptr(), buf.data_ptr() + (1 << 20), dt, odt, 2, 65, 2, 64))
    assert got["code"] == ERR_ARG and got["message"].startswith(message), got
    assert after == before, "a refused call moved the plan"


if __name__ == "__main__":
    for k in SWITCHES:
        if k != "SKIMI_ATTN_Q64" or "--q32-rows" not in sys.argv:
            os.environ.pop(k, None)
    if "--q32-rows" in sys.argv:
        print(json.dumps(run_q32_rows()))
    else:
        table = {}
        for name, r in TABLE.items():
            plan, written, out, qkv = launch(r)
            check_numbers(r, written, out, qkv)
            table[name] = dict(plan=plan, written=written)
        table.update(run_q32_child())
        for name, inner in STRIDED.items():
            r, plan, packed_plan, out, packed, qkv = launch_strided(inner)
            assert torch.equal(out, packed)
            table[name] = dict(plan=plan)
        for name, go in _refusals().items():
            got, before, after = run_refusal(go)
            assert after == before, name
            table[name] = got
        print(json.dumps(table, indent=1))
