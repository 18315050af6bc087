"""GPU: the scene-cloud kernels (csrc/scene.hip; geometry.scene_point_cloud) and their use in
CameraHead.reconstruct_batch(scene=True), against the float64 restatement of tests/scene_restated.py.

Bounds: the kept count, the kept vertices (align=False), the colours and the NaN / non-finite counts are exact; the
threshold within 2 float64 ulp (both sides evaluate the same lerp on the same two float32 order statistics); lower,
upper and scale within 1e-12 (1 + |x|) (a lerp and a 3-term norm in float64); the transform within 1e-12 (adjugate
inverse against LAPACK on well-conditioned cameras); aligned vertices within one float32 ulp (a float64 affine map
rounded once to float32, the two sums associated differently)."""
import json

import numpy as np
import pytest
import torch

import scene_restated as ref
from skiing_analysis_pytorch_amd import formats, geometry, infer, vggt, weights as W
from skiing_analysis_pytorch_amd._lib import PREC_BF16X3

pytestmark = pytest.mark.gpu


def _extrinsics(rng, B, S):
    E = np.zeros((B, S, 3, 4), np.float32)
    for b in range(B):
        for s in range(S):
            q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
            E[b, s, :, :3] = q * 1.1 + rng.normal(0, 0.02, (3, 3))   # near a scaled rotation, not orthonormal
            E[b, s, :, 3] = rng.normal(0, 2.0, 3)
    return E


def _scene(rng, B, S, H, W, nchw=True):
    points = rng.normal(0.0, 2.0, (B, S, H, W, 3)).astype(np.float32)
    conf = (1.0 + np.exp(rng.normal(size=(B, S, H, W)))).astype(np.float32)
    images = rng.random((B, S, 3, H, W) if nchw else (B, S, H, W, 3)).astype(np.float32)
    return points, conf, images, _extrinsics(rng, B, S)


def _run(points, conf, images, extrinsic, **kw):
    dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (points, conf, images, extrinsic)]
    return geometry.scene_point_cloud(*dev, **kw)


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.tobytes() == want.tobytes(), what


def _close(got, want, what, tol=1e-12):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: {got} vs {want}"
    with np.errstate(invalid="ignore"):   # inf against inf is settled by got == want
        ok = np.isnan(want) | (got == want) | (np.abs(got - want) <= tol * (1 + np.abs(want)))
    assert ok.all(), f"{what}: {got} vs {want}"


def _check(arrays, align=False, **kw):
    """every scene of a batched call against the restatement of that scene"""
    points, conf, images, extrinsic = arrays
    raw = _run(*arrays, align=False, **kw)
    out = _run(*arrays, align=True, **kw) if align else raw
    torch.cuda.synchronize()
    cap = raw.xyz.shape[1]
    wants = []
    for b in range(points.shape[0]):
        want = ref.scene_cloud(points[b], conf[b], images[b], extrinsic[b], align=False, **kw)
        wants.append(want)
        tag = f"scene {b} {kw}"
        count = int(raw.count[b])
        assert count == want["count"], f"{tag}: count {count} vs {want['count']}"
        k = min(count, cap)
        _same(raw.xyz[b, :k].cpu().numpy(), want["xyz"], f"{tag}: kept vertices")
        _same(raw.rgb[b, :k].cpu().numpy(), want["rgb"], f"{tag}: colours")
        assert int(raw.n_nan_conf[b]) == want["n_nan_conf"] and int(raw.n_nonfinite[b]) == want["n_nonfinite"], tag
        thr, wthr = float(raw.threshold[b]), want["threshold"]
        assert (np.isnan(thr) and np.isnan(wthr)) or abs(thr - wthr) <= 2 * np.spacing(abs(wthr)), f"{tag}: thr {thr} vs {wthr}"
        _close(raw.stats[b, 1:3].cpu().numpy(), [want["lo"], want["hi"]], f"{tag}: lo, hi", tol=0.0)
        _close(raw.lower[b].cpu().numpy(), want["lower"], f"{tag}: lower")
        _close(raw.upper[b].cpu().numpy(), want["upper"], f"{tag}: upper")
        _close(raw.scale[b].cpu().numpy(), want["scale"], f"{tag}: scale")
        assert np.abs(raw.transform[b].cpu().numpy() - want["transform"]).max() <= 1e-12, f"{tag}: transform"
        if align:
            wa = ref.scene_cloud(points[b], conf[b], images[b], extrinsic[b], align=True, **kw)
            got = out.xyz[b, :k].cpu().numpy()
            fin = np.isfinite(wa["xyz"]).all(axis=1) & np.isfinite(want["xyz"]).all(axis=1)
            assert (np.abs(got[fin] - wa["xyz"][fin]) <= np.spacing(np.abs(wa["xyz"][fin]))).all(), f"{tag}: aligned vertices"
            _same(out.rgb[b, :k].cpu().numpy(), want["rgb"], f"{tag}: colours (aligned call)")
            assert int(out.count[b]) == count
    return raw, wants


# ---- shapes ----
def test_under_a_wave():
    _check(_scene(np.random.default_rng(1), 1, 1, 5, 7), align=True)
    _check(_scene(np.random.default_rng(2), 1, 1, 5, 7), conf_thres=10.0)


def test_several_workgroups_and_a_ragged_tail():
    tile = geometry.scene_launch(1)[1]
    n = 2 * tile + 37
    assert geometry.scene_launch(n) == (3, tile)
    raw, wants = _check(_scene(np.random.default_rng(3), 2, 1, 1, n), align=True)
    assert 0 < wants[0]["count"] < n


@pytest.mark.parametrize("nchw", [True, False])
def test_three_views_three_scenes(nchw):
    assert geometry.scene_launch(3 * 70 * 73)[0] > 1
    _check(_scene(np.random.default_rng(4), 3, 3, 70, 73, nchw=nchw), align=True, conf_thres=33.3)


# ---- threshold ----
@pytest.mark.parametrize("q", [0.0, 0.5, 50.0, 99.9, 100.0])
def test_percentiles(q):
    raw, wants = _check(_scene(np.random.default_rng(5), 2, 2, 37, 41), conf_thres=q)
    if q == 100.0:
        assert wants[0]["count"] == 1


def _with_conf(seed, make):
    points, conf, images, extrinsic = _scene(np.random.default_rng(seed), 2, 2, 37, 41)
    rng = np.random.default_rng(seed + 100)
    conf = np.stack([make(rng, conf[b].shape) for b in range(2)]).astype(np.float32)
    return points, conf, images, extrinsic


@pytest.mark.parametrize("q", [0.5, 50.0, 99.9])
def test_threshold_on_a_tie(q):
    arrays = _with_conf(6, lambda rng, shape: 1.0 + rng.integers(0, 8, shape) * 0.25)
    raw, wants = _check(arrays, conf_thres=q)
    assert wants[0]["lo"] == wants[0]["hi"]


def test_all_confidences_equal():
    raw, wants = _check(_with_conf(7, lambda rng, shape: np.full(shape, 1.5)), conf_thres=50.0)
    assert wants[0]["count"] == 2 * 37 * 41


def test_shared_leading_digits():
    arrays = _with_conf(8, lambda rng, shape: 1.0 + rng.integers(0, 4000, shape) * 2.0 ** -23)
    _check(arrays, conf_thres=50.0)
    _check(arrays, conf_thres=99.9)


def test_negatives_zeros_and_inf():
    def make(rng, shape):
        c = rng.normal(0.0, 1.0, shape)
        flat = c.reshape(-1)
        flat[rng.random(flat.size) < 0.2] = 0.0
        flat[rng.random(flat.size) < 0.2] = -0.0
        flat[rng.random(flat.size) < 0.01] = np.inf
        flat[rng.random(flat.size) < 0.01] = -np.inf
        return c
    arrays = _with_conf(9, make)
    for q in (10.0, 50.0, 99.9, 100.0):
        _check(arrays, conf_thres=q)


def test_one_nan_confidence_empties_the_cloud():
    arrays = _with_conf(10, lambda rng, shape: 1.0 + rng.random(shape))
    arrays[1][0, 1, 3, 5] = np.nan
    raw, wants = _check(arrays, conf_thres=50.0)
    assert int(raw.count[0]) == 0 and float(raw.scale[0]) == 1.0 and int(raw.n_nan_conf[0]) == 1
    assert np.isnan(float(raw.threshold[0])) and int(raw.count[1]) > 0
    raw, wants = _check(arrays, conf_thres=0.0)   # no percentile is taken: the NaN is merely not kept
    assert int(raw.count[0]) == 2 * 37 * 41 - 1


def test_tiny_confidences_stay_out_at_zero():
    def make(rng, shape):
        c = 1.0 + rng.random(shape)
        flat = c.reshape(-1)
        flat[::3] = np.float32(1e-5)                                   # not above float32(1e-5)
        flat[1::9] = np.nextafter(np.float32(1e-5), np.float32(1))     # just above
        flat[2::9] = 0.0
        return c
    raw, wants = _check(_with_conf(11, make), conf_thres=0.0)
    assert 0 < wants[0]["count"] < 2 * 37 * 41


# ---- colours ----
@pytest.mark.parametrize("nchw", [True, False])
def test_mask_boundaries(nchw):
    rng = np.random.default_rng(12)
    points, conf, images, extrinsic = _scene(rng, 2, 2, 37, 41, nchw=False)
    levels = np.array([[5, 5, 5], [5, 5, 6], [0, 0, 16], [0, 0, 0], [241, 241, 240], [241, 241, 241], [240, 255, 255],
                       [255, 255, 255], [120, 7, 250]], np.float64)
    pick = rng.integers(0, len(levels), images.shape[:-1])
    images = ((levels[pick] + 0.5) / 255.0).astype(np.float32)   # truncates to the level
    assert np.array_equal(ref.colour_u8(images), levels[pick].astype(np.uint8))
    if nchw:
        images = np.ascontiguousarray(np.transpose(images, (0, 1, 4, 2, 3)))
    arrays = (points, conf, images, extrinsic)
    counts = []
    for black, white in ((True, False), (False, True), (True, True), (False, False)):
        raw, wants = _check(arrays, conf_thres=10.0, mask_black_bg=black, mask_white_bg=white)
        counts.append(wants[0]["count"])
    assert counts[2] < counts[0] < counts[3] and counts[2] < counts[1] < counts[3]


def test_colour_rule_out_of_range():
    points, conf, images, extrinsic = _scene(np.random.default_rng(13), 1, 1, 16, 16)
    flat = images.reshape(-1)
    flat[:16] = np.arange(16, dtype=np.float32) / np.float32(255)   # k / 255 may give k - 1
    flat[16:22] = [np.nan, -0.5, -1e-3, 256.0 / 255.0 * 1.01, np.inf, -np.inf]
    flat[22:30] = [1.0, 254.9999 / 255, 255.5 / 255, 2.0, 1e30, -0.0, 0.999999, 1.003]
    _check((points, conf, images, extrinsic), conf_thres=0.0)


# ---- kept count ----
@pytest.mark.parametrize("k", [0, 1, 2])
def test_few_kept(k):
    points, conf, images, extrinsic = _scene(np.random.default_rng(14), 2, 1, 9, 11)
    conf[0] = 1e-6
    conf[0].reshape(-1)[np.array([17, 60][:k], dtype=np.int64)] = 1.0
    raw, wants = _check((points, conf, images, extrinsic), align=True, conf_thres=0.0)
    assert int(raw.count[0]) == k
    if k == 0:
        assert float(raw.scale[0]) == 1.0 and np.isnan(raw.lower[0].cpu().numpy()).all()


def test_kept_vertex_with_nan_coordinate():
    points, conf, images, extrinsic = _scene(np.random.default_rng(15), 2, 2, 37, 41)
    order = np.argsort(conf[0].reshape(-1))
    points[0].reshape(-1, 3)[order[-1], 1] = np.nan     # the most confident pixels are kept
    points[0].reshape(-1, 3)[order[-2], 0] = np.inf
    points[0].reshape(-1, 3)[order[0], 2] = np.nan      # dropped: does not count
    raw, wants = _check((points, conf, images, extrinsic), conf_thres=50.0)
    assert int(raw.n_nonfinite[0]) == 2 and np.isnan(float(raw.scale[0]))
    lower = raw.lower[0].cpu().numpy()
    assert np.isnan(lower[1]) and np.isfinite(lower[2]) and np.isfinite(float(raw.scale[1]))


# ---- capacity ----
def test_capacity_below_count():
    arrays = _scene(np.random.default_rng(16), 2, 2, 70, 73)
    n = 2 * 70 * 73
    full, wants = _check(arrays, conf_thres=50.0)
    cap = wants[0]["count"] // 3
    assert cap > 256
    xyz = torch.full((2, cap + 8, 3), -7.5, dtype=torch.float32, device="cuda")
    rgb = torch.full((2, cap + 8, 3), 99, dtype=torch.uint8, device="cuda")
    dev = [torch.from_numpy(a).cuda() for a in arrays]
    # the kernels see capacity `cap`; the 8 rows behind each scene's block are the next scene's or the buffer's end
    out = geometry.scene_point_cloud(*dev, conf_thres=50.0, align=False, capacity=cap,
                                     out=(xyz.view(-1)[:2 * cap * 3].view(2, cap, 3), rgb.view(-1)[:2 * cap * 3].view(2, cap, 3)))
    torch.cuda.synchronize()
    assert (xyz.view(-1)[2 * cap * 3:] == -7.5).all() and (rgb.view(-1)[2 * cap * 3:] == 99).all()
    for b in range(2):
        assert int(out.count[b]) == wants[b]["count"] > cap
        _same(out.xyz[b].cpu().numpy(), wants[b]["xyz"][:cap], "first cap rows")
        _same(out.rgb[b].cpu().numpy(), wants[b]["rgb"][:cap], "first cap colours")
    _same(out.stats.cpu().numpy(), full.stats.cpu().numpy(), "stats are those of all kept vertices")
    # a scene that keeps fewer than cap leaves its rows beyond count untouched
    conf = arrays[1].copy()
    conf[1].reshape(-1)[100:] = 1e-6
    xyz.fill_(-7.5)
    out = geometry.scene_point_cloud(dev[0], torch.from_numpy(conf).cuda(), dev[2], dev[3], conf_thres=0.0, align=False,
                                     capacity=cap + 8, out=(xyz, rgb))
    torch.cuda.synchronize()
    assert int(out.count[1]) == 100 and (xyz[1, 100:] == -7.5).all() and int(out.count[0]) == n


# ---- batching ----
def test_batched_scenes_equal_single_calls_and_reruns():
    arrays = _scene(np.random.default_rng(17), 3, 3, 70, 73)
    arrays[0][1, 0, 0, 0, 0] = np.nan
    batch = _run(*arrays, conf_thres=50.0)
    again = _run(*arrays, conf_thres=50.0)
    torch.cuda.synchronize()
    for b in range(3):
        one = _run(*(a[b:b + 1] for a in arrays), conf_thres=50.0)
        k = int(batch.count[b])
        assert k == int(one.count[0]) == int(again.count[b]) > 0
        for name in ("xyz", "rgb"):
            x = getattr(batch, name)[b, :k].cpu().numpy()
            _same(getattr(one, name)[0, :k].cpu().numpy(), x, f"{name} alone")
            _same(getattr(again, name)[b, :k].cpu().numpy(), x, f"{name} rerun")
        for name in ("stats", "transform"):
            x = getattr(batch, name)[b].cpu().numpy()
            _same(getattr(one, name)[0].cpu().numpy(), x, f"{name} alone")
            _same(getattr(again, name)[b].cpu().numpy(), x, f"{name} rerun")


def test_arguments():
    p, c, im, E = (torch.from_numpy(a).cuda() for a in _scene(np.random.default_rng(18), 1, 1, 5, 7))
    with pytest.raises(ValueError):
        geometry.scene_point_cloud(p, c, im, E, conf_thres=100.5)
    with pytest.raises(ValueError):
        geometry.scene_point_cloud(p, c, im, E, conf_thres=-1.0)
    with pytest.raises(ValueError):
        geometry.scene_point_cloud(p, c, im, E, capacity=0)
    with pytest.raises(ValueError):
        geometry.scene_point_cloud(p, c[:, :, :4], im, E)
    with pytest.raises(Exception, match="device"):
        geometry.scene_point_cloud(p.cpu(), c, im, E)


# ---- entry point ----
@pytest.fixture(scope="module")
def tiny_model(golden_dir):
    g = np.load(golden_dir / "vggt_tiny_conv.npz")
    cfg = W.VGGTConfig(**json.loads(str(g["cfg_json"])))
    m = vggt.VGGT(config=cfg, prec=PREC_BF16X3, head_prec=PREC_BF16X3)
    m.load_state_dict(W.make_vggt_state_dict(cfg, seed=0))
    return m


@pytest.mark.parametrize("mode", ["All", "Predicted Pointmap"])
def test_reconstruct_batch_writes_the_scene_glb(tiny_model, tmp_path, mode):
    m = tiny_model
    rng = np.random.default_rng(19)
    steps = [[torch.from_numpy(rng.integers(0, 256, (135, 240, 3), dtype=np.uint8)) for _ in range(2)] for _ in range(2)]
    conf = {"infer": {"gpu": 0}, "conf_thres": 50.0, "prediction_mode": mode}
    plain = infer.CameraHead(conf, tmp_path / "plain", model=m).reconstruct_batch([3, 4], steps)
    head = infer.CameraHead(conf, tmp_path / "scene", model=m)
    recs = head.reconstruct_batch([3, 4], steps, scene=True)
    cloud = head.last_scene
    for b, fid in enumerate((3, 4)):
        for x, y in zip(recs[b], plain[b]):
            if isinstance(x, list):
                assert all(np.array_equal(u, v) for u, v in zip(x, y))
            else:
                _same(x, y, "returned tuple")
        a = np.load(tmp_path / "plain" / f"frame_{fid:04d}" / "predictions.npz")
        z = np.load(tmp_path / "scene" / f"frame_{fid:04d}" / "predictions.npz")
        assert sorted(a.files) == sorted(z.files)
        for key in a.files:
            _same(z[key], a[key], key)
        glb = tmp_path / "scene" / f"frame_{fid:04d}" / f"scene_conf50.0_mode{mode.replace(' ', '_')}.glb"
        assert glb.exists() and not list((tmp_path / "plain").glob("*/*.glb"))
        xyz, rgb = formats.read_glb_points(glb)
        k = int(cloud.count[b])
        assert 0 < k <= cloud.xyz.shape[1]
        _same(xyz, cloud.xyz[b, :k].cpu().numpy(), "GLB vertices")
        _same(rgb, cloud.rgb[b, :k].cpu().numpy(), "GLB colours")
    # the cloud is the restatement's on the maps the head kept on the device
    if mode == "All":
        wp = head.last_world_points[0].cpu().numpy()
        assert int(cloud.count[0]) >= wp.shape[0] * wp.shape[1] * wp.shape[2] // 2
