"""CPU: the float64 restatement of the VideoPose3D streaming layers (tests/vp3d_stream_restated.py) against itself,
against torch's own bf16, and its forward against the float32 oracle and the dense restatement."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import vp3d_dense_restated as RD  # noqa: E402
import vp3d_stream_restated as R  # noqa: E402

from oracle import vp3d_oracle  # noqa: E402
from skiing_analysis_pytorch_amd import weights as W  # noqa: E402


def _rng(seed):
    return np.random.default_rng(seed)


def test_bf16_rounding_is_torchs():
    g = _rng(0)
    x = np.concatenate([g.standard_normal(4096).astype(np.float32) * np.float32(2.0) ** g.integers(-20, 20, 4096).astype(np.float32),
                        # ties: exactly half way between two bf16 values, even and odd neighbours
                        np.array([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(2.0 + 2.0 ** -7), 0.0, -0.0, 2.0 ** -130],
                                 np.float32)])
    ours = R.bf16_value(R.bf16_bits(x))
    theirs = torch.from_numpy(x).to(torch.bfloat16).to(torch.float32).numpy()
    assert np.array_equal(ours.view(np.uint32), theirs.view(np.uint32))


def test_split_identities_random():
    g = _rng(1)
    x = (g.standard_normal(20000) * 2.0 ** g.integers(-12, 12, 20000)).astype(np.float32)
    hi, lo = R.split(x)
    x64 = x.astype(np.float64)
    # both halves are bf16 values
    for h in (hi, lo):
        assert np.array_equal(R.bf16_value(R.bf16_bits(h)).view(np.uint32), h.view(np.uint32))
    assert (np.abs(x64 - hi) <= R.UB * np.abs(x64)).all()                      # |x - hi| <= 2^-8 |x|
    assert (np.abs(lo.astype(np.float64)) <= R.UB * (1 + R.UB) * np.abs(x64)).all()
    assert (np.abs(x64 - hi - lo.astype(np.float64)) <= R.UB ** 2 * np.abs(x64)).all()   # |x - hi - lo| <= 2^-16 |x|


def test_split_identities_dyadic():
    """a + b 2^-9 with a in {+-1, +-2, +-3}, b in {-1, 0, 1}: hi = a and lo = b 2^-9 exactly (and 0 -> 0, 0)"""
    a = np.array([1, -1, 2, -2, 3, -3], np.float32)
    b = np.array([-1, 0, 1], np.float32)
    x = (a[:, None] + b[None, :] * np.float32(2.0 ** -9)).astype(np.float32)
    hi, lo = R.split(x)
    assert np.array_equal(hi, np.broadcast_to(a[:, None], x.shape))
    assert np.array_equal(lo, np.broadcast_to(b[None, :] * np.float32(2.0 ** -9), x.shape))
    z = R.split(np.zeros(3, np.float32))
    assert not z[0].any() and not z[1].any()
    # torch agrees
    th = torch.from_numpy(x).to(torch.bfloat16).to(torch.float32)
    assert np.array_equal(th.numpy(), hi)
    assert np.array_equal((torch.from_numpy(x) - th).to(torch.bfloat16).to(torch.float32).numpy(), lo)


@pytest.mark.parametrize("rows,K", [(1, 32), (16, 32), (17, 96), (45, 160), (100, 64)])
def test_pack_unpack_round_trip(rows, K):
    g = _rng(rows * 1000 + K)
    x = g.standard_normal((rows, K)).astype(np.float32)
    rec = R.pack(x)
    assert rec.shape == (-(-rows // 16), K // 32, 2, 4, 16, 8) and rec.dtype == np.uint16
    hi, lo = R.unpack(rec, rows, K)
    eh, el = R.split(x)
    assert np.array_equal(hi, eh) and np.array_equal(lo, el)
    # the documented index formula, element by element
    flat = rec.reshape(-1)
    for r, k in [(0, 0), (rows - 1, K - 1), (rows // 2, K // 3), (min(rows - 1, 15), 31), (rows - 1, 8)]:
        i = R.record_index(r, k, K)
        assert R.bf16_value(flat[i]) == eh[r, k] and R.bf16_value(flat[i + 512]) == el[r, k]
    # rows past the matrix are zero
    full_hi, _ = R.unpack(rec, rec.shape[0] * 16, K)
    assert not full_hi[rows:].any()


def test_references_a_and_b():
    """A and B differ by the dropped term and the second split error, within 3 * 2^-16 sum |w| |x|; on bf16-exact
    operands they coincide."""
    g = _rng(5)
    Wt = g.standard_normal((16, 3, 32)).astype(np.float32)
    X = g.standard_normal((2, 21, 32)).astype(np.float32)
    bias = g.standard_normal(16).astype(np.float32)
    r = R.conv(Wt, X, bias, dil=2, relu=False)
    assert r["A"].shape == (2, 17, 16)
    d = np.abs(r["A"] - r["B"])
    assert d.max() > 0 and (d <= 3 * 2.0 ** -16 * r["SB"]).all()
    Wh, Xh = R.split(Wt)[0], R.split(X)[0]
    r = R.conv(Wh, Xh, bias, dil=2, relu=True)
    assert np.array_equal(r["A"], r["B"])
    # against torch's conv1d in float64
    ref = torch.nn.functional.conv1d(torch.from_numpy(Xh).double().permute(0, 2, 1),
                                     torch.from_numpy(Wh).double().permute(0, 2, 1), torch.from_numpy(bias).double(),
                                     dilation=2).relu().permute(0, 2, 1).numpy()
    assert np.abs(r["B"] - ref).max() < 1e-12
    # residual slice
    res = g.standard_normal((2, 30, 16)).astype(np.float32)
    rr = R.conv(Wh, Xh, bias, dil=2, relu=True, resid=res, resid_off=5)
    assert np.abs(rr["B"] - (ref + res[:, 5:22])).max() < 1e-12


@pytest.mark.parametrize("dense", [False, True])
@pytest.mark.parametrize("causal", [False, True])
def test_forward_matches_oracle_and_dense_restatement(dense, causal):
    fw = [3, 3, 3]
    sd = W.make_vp3d_state_dict(seed=2, joints_out=12, filter_widths=fw, channels=96, dense=dense)
    rf = R.receptive_field(fw)
    assert rf == 27 == RD.receptive_field(fw)
    x = torch.randn(2, rf + 9, 17, 2, generator=torch.Generator().manual_seed(4))
    out, bound = R.forward(sd, x.numpy(), fw, causal=causal, dense=dense, with_bound=True)
    assert out.shape == (2, 10, 12, 3) and bound.shape == out.shape
    assert (bound > 0).all() and np.isfinite(bound).all()
    scale = max(1.0, np.abs(out).max())
    if dense:
        ref64 = RD.forward(sd, x, fw, causal).numpy()
        assert np.abs(out - ref64).max() < 1e-12 * scale
    else:
        with torch.no_grad():
            ref32 = vp3d_oracle.temporal_model_forward(sd, x, fw, causal=causal).numpy()
        assert np.abs(out - ref32).max() < 2e-5 * scale       # float32 accuracy of the oracle
        assert (np.abs(out - ref32) <= bound).all()            # and a float32 evaluation sits inside the kernel's bound
