"""CPU: the scene cloud's rules (tests/scene_restated.py) against the reference's own predictions_to_glb
(tests/golden/scene_cloud.npz, written by tools/make_goldens.py scene), the colour rule, the GLB writer / reader, and
the branch choice of infer.predictions_to_glb_points with the restatement standing in for the device call.

The scale bound: the reference takes its percentiles with NumPy's float32 lerp, the rules in float64.  On the golden's
eight argument sets the worst relative difference between 0.1 * scale and the recorded cone height is 1.16e-7
(profiles/scene_cloud.md; float32 rounding inside NumPy's percentile); the bound is 4 x that.  The set that keeps one
vertex has scale 0 on both sides."""
import json
import struct

import numpy as np
import pytest
import torch

import scene_restated as ref
from skiing_analysis_pytorch_amd import formats, geometry, infer

SCALE_RTOL = 4 * 1.16e-7
assert SCALE_RTOL <= 1e-5


@pytest.fixture(scope="module")
def golden(golden_dir):
    g = np.load(golden_dir / "scene_cloud.npz")
    return g, json.loads(str(g["sets_json"]))


@pytest.fixture()
def restated_device_call(monkeypatch):
    """geometry.scene_point_cloud replaced by the restatement on host tensors; records the arguments it was given"""
    calls = []

    def stub(points, conf, images, extrinsic, **kw):
        calls.append(dict(kw, points=points, conf=conf, images=images, extrinsic=extrinsic))
        return [ref.scene_cloud(points[b].numpy(), conf[b].numpy(), images[b].numpy(), extrinsic[b].numpy(), align=False, **kw)
                for b in range(points.shape[0])]

    monkeypatch.setattr(geometry, "scene_point_cloud", stub)
    return calls


def _preds(g):
    return {k: torch.from_numpy(g[k]) for k in ("world_points", "world_points_conf", "world_points_from_depth", "depth_conf",
                                                "images", "extrinsic")}


def test_restatement_matches_the_reference(golden, restated_device_call):
    g, sets = golden
    assert len(sets) == 8
    worst = 0.0
    for i, kw in enumerate(sets):
        got = infer.predictions_to_glb_points(_preds(g), **kw)[0]
        want_v, want_c = g[f"s{i}_vertices"], g[f"s{i}_colors"]
        assert got["xyz"].dtype == np.float32 and got["xyz"].tobytes() == want_v.tobytes(), f"set {i} {kw}: kept vertices"
        assert np.array_equal(got["rgb"], want_c), f"set {i} {kw}: colours"
        assert np.abs(got["transform"] - g[f"s{i}_transform"]).max() <= 1e-12, f"set {i}: transform"
        radius, height = g[f"s{i}_cone"]
        assert (height == 0) == (got["scale"] == 0), f"set {i} {kw}: scale {got['scale']} against cone height {height}"
        rel = 0.0 if height == 0 else max(abs(0.1 * got["scale"] - height) / height, abs(0.05 * got["scale"] - radius) / radius)
        print(f"set {i} {kw}: count {got['count']}, scale {got['scale']!r}, relative difference to the cone {rel:.3e}")
        worst = max(worst, rel)
        assert rel <= SCALE_RTOL, f"set {i} {kw}: scale {got['scale']} against cone height {height}"
    print(f"worst relative scale difference {worst:.3e}")


def test_colour_rule_matches_numpy_for_every_level():
    for x in ((np.arange(256) / 255.0).astype(np.float32), np.arange(256, dtype=np.float32) / np.float32(255.0),
              np.nextafter((np.arange(256) / 255.0).astype(np.float32), np.float32(-1))):   # the last: every k >= 1 gives k - 1
        assert np.array_equal(ref.colour_u8(x), (x * 255).astype(np.uint8))
    assert np.array_equal(ref.colour_u8(np.array([np.nan, -0.3, -1e9, 256 / 255 * 1.001, 7.0, np.inf], np.float32)),
                          np.array([0, 0, 0, 255, 255, 255], np.uint8))


def test_percentile_rule_matches_numpy_at_test_sizes():
    rng = np.random.default_rng(0)
    for n in (1, 2, 35, 384, 3034):
        x = (1 + np.exp(rng.normal(size=n))).astype(np.float32)
        for q in (0.0, 0.5, 5.0, 10.0, 50.0, 95.0, 99.9, 100.0):
            got = ref.percentile_linear(x, q)[0]
            want = np.percentile(x.astype(np.float64), q)
            assert abs(got - want) <= 4 * np.spacing(abs(want)), (n, q)
    assert np.isnan(ref.percentile_linear(np.array([1.0, np.nan], np.float32), 50.0)[0])
    z = ref.percentile_linear(np.array([0.0, -0.0, 0.0, -0.0], np.float32), 0.0)
    assert np.signbit(z[1]) and np.signbit(ref.percentile_linear(np.array([0.0, -0.0], np.float32), 100.0)[2]) == False  # noqa: E712


def test_glb_round_trip(tmp_path):
    rng = np.random.default_rng(1)
    for n in (1, 2, 3, 7, 1000):   # 16 n is a multiple of 4; the JSON length varies with n
        xyz = rng.normal(0, 3, (n, 3)).astype(np.float32)
        rgb = rng.integers(0, 256, (n, 3)).astype(np.uint8)
        path = formats.write_glb_points(tmp_path / f"c{n}.glb", xyz, rgb)
        x2, c2 = formats.read_glb_points(path)
        assert x2.dtype == np.float32 and c2.dtype == np.uint8
        assert x2.tobytes() == xyz.tobytes() and c2.tobytes() == rgb.tobytes()
        data = path.read_bytes()
        magic, version, total = struct.unpack_from("<III", data, 0)
        assert magic == 0x46546C67 and data[:4] == b"glTF" and version == 2 and total == len(data)
        jlen, jkind = struct.unpack_from("<II", data, 12)
        assert jkind == 0x4E4F534A and jlen % 4 == 0
        js = data[20:20 + jlen]
        blen, bkind = struct.unpack_from("<II", data, 20 + jlen)
        assert bkind == 0x004E4942 and blen % 4 == 0 and 28 + jlen + blen == total and blen == 16 * n
        gltf = json.loads(js.decode("utf-8"))
        assert js.rstrip(b" ") + b" " * (jlen - len(js.rstrip(b" "))) == js
        prim = gltf["meshes"][0]["primitives"][0]
        assert prim["mode"] == 0 and len(gltf["meshes"]) == 1 and len(gltf["meshes"][0]["primitives"]) == 1
        pos, col = gltf["accessors"][prim["attributes"]["POSITION"]], gltf["accessors"][prim["attributes"]["COLOR_0"]]
        assert pos["componentType"] == 5126 and pos["type"] == "VEC3" and pos["count"] == n
        assert pos["min"] == [float(v) for v in xyz.min(axis=0)] and pos["max"] == [float(v) for v in xyz.max(axis=0)]
        assert col["componentType"] == 5121 and col["type"] == "VEC4" and col["normalized"] is True
        rgba = np.frombuffer(data, np.uint8, offset=28 + jlen + 12 * n, count=4 * n).reshape(n, 4)
        assert (rgba[:, 3] == 255).all() and np.array_equal(rgba[:, :3], rgb)
        assert gltf["buffers"][0]["byteLength"] == 16 * n


def test_glb_empty_cloud_is_one_white_point(tmp_path):
    path = formats.write_glb_points(tmp_path / "empty.glb", np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint8))
    xyz, rgb = formats.read_glb_points(path)
    assert np.array_equal(xyz, np.array([[1, 0, 0]], np.float32)) and np.array_equal(rgb, np.array([[255, 255, 255]], np.uint8))
    with pytest.raises(ValueError):
        formats.write_glb_points(tmp_path / "bad.glb", np.zeros((2, 3)), np.zeros((3, 3)))
    (tmp_path / "junk.glb").write_bytes(b"not a glb file at all.....")
    with pytest.raises(ValueError):
        formats.read_glb_points(tmp_path / "junk.glb")


def test_glb_bounds_skip_non_finite(tmp_path):
    xyz = np.array([[0, 1, 2], [np.nan, -3, np.inf], [4, 5, -6]], np.float32)
    path = formats.write_glb_points(tmp_path / "nf.glb", xyz, np.zeros((3, 3), np.uint8))
    data = path.read_bytes()
    jlen = struct.unpack_from("<I", data, 12)[0]
    pos = json.loads(data[20:20 + jlen])["accessors"][0]   # strict JSON: no NaN / Infinity tokens
    assert pos["min"] == [0.0, -3.0, -6.0] and pos["max"] == [4.0, 5.0, 2.0]
    assert formats.read_glb_points(path)[0].tobytes() == xyz.tobytes()


def test_branch_choice(golden, restated_device_call):
    g, _ = golden
    calls = restated_device_call
    preds = _preds(g)

    def used(**kw):
        calls.clear()
        infer.predictions_to_glb_points(**kw)
        (c,) = calls
        return c

    c = used(preds=preds, conf_thres=50.0, prediction_mode="Predicted Pointmap")
    assert torch.equal(c["points"][0], preds["world_points"]) and torch.equal(c["conf"][0], preds["world_points_conf"])
    assert c["conf_thres"] == 50.0 and c["mask_black_bg"] is False and c["mask_white_bg"] is False
    for mode in ("All", "Depthmap and Camera Branch", "pointmap"):   # the test is case-sensitive, as the reference's
        c = used(preds=preds, conf_thres=50.0, prediction_mode=mode)
        assert torch.equal(c["points"][0], preds["world_points_from_depth"]) and torch.equal(c["conf"][0], preds["depth_conf"])
    no_wp = {k: v for k, v in preds.items() if not k.startswith("world_points") or k == "world_points_from_depth"}
    c = used(preds=no_wp, conf_thres=50.0, prediction_mode="Predicted Pointmap")   # falls back to the depth branch
    assert torch.equal(c["points"][0], preds["world_points_from_depth"]) and torch.equal(c["conf"][0], preds["depth_conf"])
    no_conf = {k: v for k, v in preds.items() if k not in ("world_points_conf", "depth_conf")}
    for mode in ("Predicted Pointmap", "All"):
        c = used(preds=no_conf, conf_thres=50.0, prediction_mode=mode)
        assert c["conf"].shape == (1, 2, 12, 16) and (c["conf"] == 1).all()
    c = used(preds=preds, conf_thres=None, prediction_mode="All")
    assert c["conf_thres"] == 10.0
    c = used(preds=preds, conf_thres=50.0, prediction_mode="All", mask_black_bg=True, mask_white_bg=True)
    assert c["mask_black_bg"] is True and c["mask_white_bg"] is True
    # a batch of steps goes through as it is
    batch = {k: torch.stack([v, v]) for k, v in preds.items()}
    c = used(preds=batch, conf_thres=50.0, prediction_mode="All")
    assert c["points"].shape == (2, 2, 12, 16, 3) and c["images"].shape == (2, 2, 3, 12, 16)


def test_filter_by_frames_and_mask_sky(golden, restated_device_call):
    g, _ = golden
    calls = restated_device_call
    preds = _preds(g)
    infer.predictions_to_glb_points(preds, 50.0, "All", filter_by_frames="1: second view")
    c = calls[-1]
    assert c["points"].shape == (1, 1, 12, 16, 3) and torch.equal(c["points"][0, 0], preds["world_points_from_depth"][1])
    assert torch.equal(c["images"][0, 0], preds["images"][1]) and torch.equal(c["extrinsic"][0, 0], preds["extrinsic"][1])
    for everything in ("all", "All", "no number"):
        infer.predictions_to_glb_points(preds, 50.0, "All", filter_by_frames=everything)
        assert calls[-1]["points"].shape == (1, 2, 12, 16, 3)
    with pytest.raises(IndexError):
        infer.predictions_to_glb_points(preds, 50.0, "All", filter_by_frames="2:")
    with pytest.raises(NotImplementedError):
        infer.predictions_to_glb_points(preds, 50.0, "All", mask_sky=True)
    with pytest.raises(ValueError):
        infer.predictions_to_glb_points([preds], 50.0, "All")


def test_restatement_rejects_q_outside_the_range():
    x = np.zeros((1, 2, 2, 3), np.float32)
    with pytest.raises(ValueError):
        ref.scene_cloud(x, np.ones((1, 2, 2), np.float32), x, np.eye(3, 4, dtype=np.float32)[None], conf_thres=101.0)
