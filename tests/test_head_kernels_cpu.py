"""CPU: the float64 restatements of the VGGT head / track-head helper kernels (head_kernels_restated.py) against
independent implementations -- torch's own operators and the oracle -- so that a restatement cannot agree with a kernel
by construction.  No GPU, no library call."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import head_kernels_restated as R
from oracle import vggt_oracle as O

U = R.U


def _rng(seed):
    return np.random.default_rng(seed)


RESIZE_SHAPES = [((3, 5), (7, 12)), ((4, 4), (4, 4)), ((9, 9), (4, 5)), ((1, 6), (5, 6)), ((6, 1), (6, 3)), ((5, 7), (1, 1)),
                 ((10, 10), (37, 37)), ((37, 37), (74, 74))]


@pytest.mark.parametrize("src,dst", RESIZE_SHAPES)
def test_resize_matches_float32_interpolate(src, dst):
    """float32 F.interpolate rounds its lerp in fp32 (8 roundings on the absolute-value lerp); its INDICES are what
    the restatement must share, and an index off by one ulp shows far above that"""
    x = _rng(1).standard_normal((2, *src, 4)).astype(np.float32)
    ref = F.interpolate(torch.from_numpy(x).permute(0, 3, 1, 2), size=dst, mode="bilinear", align_corners=True)
    v, mag = R.resize(x, *dst)
    err = np.abs(ref.permute(0, 2, 3, 1).numpy().astype(np.float64) - v)
    assert (err <= 8 * U * mag).all(), (err / np.maximum(mag, 1e-30)).max() / U
    if src == dst:
        assert np.array_equal(v, x.astype(np.float64))


def test_resize_float32_indices_differ_from_float64():
    """37 -> 74: float64 interpolate is NOT the definition (the float32 scale moves the weights by ~1e-6)"""
    x = _rng(2).standard_normal((1, 37, 37, 4)).astype(np.float32)
    ref64 = F.interpolate(torch.from_numpy(x).double().permute(0, 3, 1, 2), size=(74, 74), mode="bilinear", align_corners=True)
    v, mag = R.resize(x, 74, 74)
    err = np.abs(ref64.permute(0, 2, 3, 1).numpy() - v)
    assert (err > 8 * U * mag).any() and err.max() < 1e-4


def test_resize_uv_and_layernorm():
    x = _rng(3).standard_normal((2, 3, 5, 8))
    tabx, taby = _rng(4).standard_normal((12, 4)), _rng(5).standard_normal((7, 4))
    v, mag = R.resize(x, 7, 12, tabx, taby)
    v0, _ = R.resize(x, 7, 12)
    assert np.array_equal(v[1, 3, 5, :4], v0[1, 3, 5, :4] + tabx[5]) and np.array_equal(v[1, 3, 5, 4:], v0[1, 3, 5, 4:] + taby[3])
    g, b = _rng(6).standard_normal(8), _rng(7).standard_normal(8)
    out, _, _ = R.layernorm(v, g, b, 1e-5)
    ref = F.layer_norm(torch.from_numpy(v), (8,), torch.from_numpy(g), torch.from_numpy(b), 1e-5).numpy()
    assert np.abs(out - ref).max() < 1e-12


def test_16bit_helpers():
    x = torch.from_numpy(_rng(8).standard_normal(4096).astype(np.float32) * 37.0)
    bits = R.bf16_rne_bits(x.numpy())
    assert np.array_equal(bits, x.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16))
    assert np.array_equal(R.decode16(bits, False), x.to(torch.bfloat16).double().numpy())
    h = x.to(torch.float16)
    assert np.array_equal(R.decode16(h.view(torch.int16).numpy().view(np.uint16), True), h.double().numpy())
    for f16, dt in ((False, torch.bfloat16), (True, torch.float16)):
        err = np.abs(x.to(dt).double().numpy() - x.double().numpy())
        assert (err <= R.half_ulp16(x.double().numpy(), f16)).all()
    slot, lo = R.plane_slots(64, True)
    assert lo == 32 and slot[31] == 31 and slot[32] == 64 and slot[63] == 95
    assert R.plane_slots(16, False)[1] == 16


HAND_COORDS = [(3.3, 1.7), (2.0, 3.0), (8.0, 4.0), (-3.5, 2.0), (19.0, -1.0), (-0.5, -0.25), (7.25, 0.5), (0.0, 3.999)]   # (H, W) = (5, 9)


def test_border_sampler_matches_oracle():
    fmap = _rng(9).standard_normal((2, 5, 9, 3)).astype(np.float32)
    coords = np.stack([np.array(HAND_COORDS, np.float32), np.array(HAND_COORDS[::-1], np.float32)])
    ref = O.sample_features4d(torch.from_numpy(fmap).double().permute(0, 3, 1, 2), torch.from_numpy(coords).double()).numpy()
    out, mag, _ = R.sample_border(fmap, coords)
    assert np.abs(out - ref).max() < 1e-13
    assert np.array_equal(out[0, 2], fmap[0, 4, 8].astype(np.float64))        # exactly (W-1, H-1)
    assert np.array_equal(out[0, 4], fmap[0, 0, 8].astype(np.float64))        # (W+10, -1) clamps to the corner
    assert (mag >= np.abs(out)).all()


@pytest.mark.parametrize("D", [196, 388])
def test_pos_embed_matches_oracle(D):
    coords = np.array(HAND_COORDS, np.float32)
    pe = O.sincos_pos_embed_2d(D, 5, 9)
    assert pe.dtype == torch.float32
    ref = O.sample_features4d(pe.double(), torch.from_numpy(coords).double()[None]).numpy()[0]
    out, _, _ = R.pos_embed_sample(coords, 5, 9, D)
    assert np.abs(out - ref).max() < 1e-13
    # the table itself, bit for bit after the float32 rounding
    assert np.array_equal(R.pos_embed_table(D, 9), pe[0, :D // 2, 0, :].T.double().numpy())


@pytest.mark.parametrize("E", [32, 64])
def test_flow_embedding_matches_oracle(E):
    """the oracle evaluates sin / cos in float32: one rounding of a value <= 1, and libm's own ulp"""
    flow = (_rng(10).uniform(-20, 20, (24, 2))).astype(np.float32)
    ref = O.get_2d_embedding(torch.from_numpy(flow)[None], E)[0].double().numpy()
    out = R.flow_embedding(flow, E)
    assert np.abs(out - ref).max() <= 2 * U
    assert np.array_equal(out[:, 0], np.zeros(24)) and np.array_equal(out[:, 1], np.ones(24))   # k = 0


def test_track_input_layout():
    S, L, B_N = 4, 64, 3
    rows, D = B_N * S, 3 * L + 4
    g = _rng(11)
    coords = g.uniform(0, 100, (rows, 2)).astype(np.float32)
    fcorr, tfeat = g.standard_normal((rows, L)).astype(np.float32), g.standard_normal((rows, L)).astype(np.float32)
    pos, qrt = g.standard_normal((B_N, D)).astype(np.float32), g.standard_normal((2, D)).astype(np.float32)
    x, mag, trig = R.track_input(coords, fcorr, tfeat, pos, qrt, S, L, 224, 518.0)
    flows = torch.from_numpy(coords).reshape(B_N, S, 2)
    flows = flows - flows[:, :1]
    femb = torch.cat([O.get_2d_embedding(flows, L // 2), flows / 518.0, flows / 518.0], dim=-1).reshape(rows, L + 4)
    tin = torch.cat([femb, torch.from_numpy(fcorr), torch.from_numpy(tfeat)], dim=1).double()
    ref = tin + torch.from_numpy(pos).double().repeat_interleave(S, 0) + \
        torch.from_numpy(qrt).double()[(torch.arange(rows) % S != 0).long()]
    assert np.abs(x[:, :D] - ref.numpy()).max() <= 2 * U
    assert not x[:, D:].any() and trig[:, :L].all() and not trig[:, L:].any()


def test_corr_sample_matches_linear_form():
    """sampling is linear: sample(<t, f>) = <t, sample(f)>, written out tap by tap with floor and zero padding"""
    B, N, S, H, W, C, r, level = 2, 3, 2, 6, 8, 16, 1, 1
    g = _rng(12)
    rows = B * N * S
    tgt, fmap = g.standard_normal((rows, C)), g.standard_normal((B * S, H, W, C))
    coords = (g.integers(-2 * 64, (W + 1) * 64, (rows, 2)) / 64.0 * 2 ** level).astype(np.float32)
    coords[0], coords[1] = (-0.5 * 2, -0.25 * 2), ((W + 20) * 2, 0)
    out, mag = R.corr_sample(tgt, fmap, coords, N, S, r, level)
    ref = np.zeros_like(out)
    for row in range(rows):
        img = fmap[(row // (N * S)) * S + row % S]
        for i in range(3):
            for j in range(3):
                x, y = coords[row, 0] / 2.0 + i - r, coords[row, 1] / 2.0 + j - r
                x0, y0 = int(np.floor(x)), int(np.floor(y))
                acc = np.zeros(C)
                for yy, wy in ((y0, 1 - (y - y0)), (y0 + 1, y - y0)):
                    for xx, wx in ((x0, 1 - (x - x0)), (x0 + 1, x - x0)):
                        if 0 <= yy < H and 0 <= xx < W:
                            acc += img[yy, xx] * wx * wy
                ref[row, i * 3 + j] = acc @ tgt[row] / np.sqrt(C)
    assert np.abs(out - ref).max() < 1e-12
    assert not out[1].any() and (mag >= np.abs(out) - 1e-12).all()


@pytest.mark.parametrize("hw", [(6, 8), (7, 9)])
def test_avgpool_matches_torch(hw):
    x = _rng(13).standard_normal((2, *hw, 3))
    ref = F.avg_pool2d(torch.from_numpy(x).permute(0, 3, 1, 2), 2, stride=2).permute(0, 2, 3, 1).numpy()
    out, _ = R.avgpool2(x)
    assert out.shape == ref.shape and np.abs(out - ref).max() < 1e-15


def test_dpt_activation_matches_oracle():
    y = np.concatenate([_rng(14).standard_normal((64, 4)) * 3, [[0, 1e-6, -1e-6, 0], [20, -20, 100, 100], [-100, 0, 0, -100]]])
    for mode in (0, 1):
        pts, conf = R.dpt_act(y, mode)
        t = torch.from_numpy(y[:, :-1])
        ref = torch.exp(t) if mode == 0 else O.inverse_log_transform(t)
        assert np.allclose(pts, ref.numpy(), rtol=1e-15, atol=0)
        assert np.allclose(conf, (1 + torch.from_numpy(y[:, -1]).exp()).numpy(), rtol=1e-15, atol=0)
    assert R.dpt_act(np.zeros((1, 2)), 1)[0][0, 0] == 0 and R.dpt_act(np.zeros((1, 2)), 1)[1][0] == 2
    yy, mag = R.dpt_pre(np.eye(2, 32), np.full((2, 32), 0.5), np.array([1.0, -1.0]))
    assert np.array_equal(yy, [[1.5, -0.5], [1.5, -0.5]]) and np.array_equal(mag, [[1.5, 1.5], [1.5, 1.5]])


@pytest.mark.parametrize("H,W,p,Kp", [(28, 42, 14, 588), (28, 42, 14, 592), (8, 12, 4, 64)])
def test_patch_gather_matches_unfold(H, W, p, Kp):
    img = _rng(15).uniform(0, 1, (2, 3, H, W)).astype(np.float32)
    t = torch.from_numpy(img).double()
    norm = (t - torch.from_numpy(R.IMAGENET_MEAN).view(1, 3, 1, 1)) / torch.from_numpy(R.IMAGENET_STD).view(1, 3, 1, 1)
    ref = F.unfold(norm, p, stride=p).permute(0, 2, 1).reshape(-1, 3 * p * p).numpy()
    A, mag = R.patch_gather(img, p, Kp)
    assert np.abs(A[:, :3 * p * p] - ref).max() < 1e-14 and not A[:, 3 * p * p:].any()
    assert (mag >= np.abs(A)).all()


def test_small_ops():
    g = _rng(16)
    xn, x, mod = g.standard_normal((3, 8)), g.standard_normal((3, 8)), g.standard_normal((3, 24))
    out, mag = R.adaln(xn, x, mod)
    assert np.allclose(out[1, 2], mod[1, 18] * (xn[1, 2] * (1 + mod[1, 10]) + mod[1, 2]) + x[1, 2], rtol=1e-15)
    assert (mag >= np.abs(out)).all()
    d = g.standard_normal((5, 9)).astype(np.float32)
    pad = np.full((5, 16), 7.0, np.float32)
    p1, a1 = R.pose_update(d, pad, True)
    p2, a2 = R.pose_update(d, p1, False)
    assert np.array_equal(p1[:, :9], d) and np.array_equal(p2[:, :9], d + d) and (p2[:, 9:] == 7).all()
    assert (a2[:, 7:] >= 0).all() and np.array_equal(a2[:, :7], p2[:, :7])
    xt, tab = np.zeros((4, 7, 8), np.float32), g.standard_normal((2, 3, 8)).astype(np.float32)
    st = R.special_tokens(xt, tab, 2)
    assert np.array_equal(st[0, :3], tab[0]) and np.array_equal(st[1, :3], tab[1]) and np.array_equal(st[2, :3], tab[0])
    assert not st[:, 3:].any()
    q = g.uniform(0, 100, (6, 2)).astype(np.float32)
    coords, qs = R.track_init(q, 3, 4.0)
    assert np.array_equal(qs, q / np.float32(4)) and np.array_equal(coords[:, 2], qs)
    c2, pred = R.track_coord_update(coords.reshape(-1, 2), np.ones((18, 66), np.float32), qs, 3, 3, 4.0, True)
    assert np.array_equal(c2.reshape(6, 3, 2)[:, 0], qs) and np.array_equal(c2.reshape(6, 3, 2)[:, 1], qs + 1)
    assert pred.shape == (2, 3, 3, 2) and np.array_equal(pred[1, 2, 0], c2.reshape(2, 3, 3, 2)[1, 0, 2] * 4)
