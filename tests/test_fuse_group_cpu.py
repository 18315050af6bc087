"""CPU: the host restatements of the joint quality (fuse.py), the group fusion (fuse.py's functions pair by pair) and the
skeleton conversion (skeleton.py) reproduce the reference's results recorded in tests/golden/fuse_group.npz; the host-only
parts of run.fuse_camera_group (loading, truncation, naming, the .npy files) against a fake device layer; the new C entry
points refuse bad arguments before any launch.  DESIGN §2 "Joint quality", "Group fusion", "Skeleton conversion"."""
import types
import warnings

import numpy as np
import pytest
import torch

import fuse_group_cases as gc
from skiing_analysis_pytorch_amd import fuse, run, skeleton

HOST_TOL = 1e-12


def same(got, want, sentinels=()):
    """NaN patterns equal, the sentinel values exactly where the reference has them, the rest within 1e-12 (1 + |x|)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    for s in sentinels:
        assert np.array_equal(got == s, want == s), f"sentinel {s} placed differently"
    return gc.close(got, want, tol=HOST_TOL)


def test_golden_inputs_are_the_seeded_cases():
    g, q, grp = gc.golden(), gc.quality_golden_case(), gc.group_golden_case()
    assert gc.bits_equal(g["q_X"], q["X"]) and gc.bits_equal(g["q_U"], q["U"]) and np.array_equal(g["q_edges"], np.array(q["edges"]))
    assert gc.bits_equal(g["g_X"], grp["X"]) and gc.bits_equal(g["g_U"], grp["U"])
    for name, arr in gc.skeleton_golden_inputs().items():
        assert gc.bits_equal(g["sk_" + name], arr), name
    assert g["target_ids"].tolist() == skeleton.MHR70_15_IDS == list(run.GROUP_TARGET_IDS)


def test_skeleton_tables():
    from skiing_analysis_pytorch_amd.device import evaluate
    g = gc.golden()
    assert [tuple(e) for e in g["bone_edge_ids"].tolist()] == skeleton.MHR70_15_BONE_IDS
    assert tuple(skeleton.MHR70_15_EDGES) == tuple(evaluate.MHR70_15_EDGES)
    assert tuple(skeleton.H36M_EDGES) == tuple(evaluate.H36M_EDGES)
    for table, n in ((skeleton.COCO_EDGES, 17), (skeleton.H36M_EDGES, 17), (skeleton.MHR70_15_EDGES, 15)):
        assert all(0 <= a < n and 0 <= b < n and a != b for a, b in table)
        assert {j for e in table for j in e} == set(range(n)) - ({0, 1} if n == 15 else set())      # the two eyes have no bone
    assert [n for n in skeleton.MHR70_15_NAMES if n in skeleton.LEFT_JOINTS] and len(skeleton.LEFT_JOINTS) == len(skeleton.RIGHT_JOINTS) == 6


def test_quality_host_matches_reference():
    g, c = gc.golden(), gc.quality_golden_case()
    kw = dict(edges=c["edges"], width=c["width"], height=c["height"], beta_temp=c["beta_temp"], w_bone=c["w_bone"],
              w_temp=c["w_temp"], w_san=c["w_san"])
    with warnings.catch_warnings():
        warnings.simplefilter("error")                       # the all-NaN edge must not reach nanmedian
        r = fuse.compute_q_nogt(c["X"], c["U"], **kw)
        r0 = fuse.compute_q_nogt(c["X"], None, **kw)
        med = fuse.bone_median_lengths(c["X"], c["edges"])
    same(med, g["q_med"])
    same(r["med_lens"], g["q_med"])
    same(r["q_bone"], g["q_bone"], sentinels=(-1e9, -100.0))
    same(r["q_temp"], g["q_temp"], sentinels=(-1e9, 0.0))
    same(r["q_san"], g["q_san"], sentinels=(-50.0, 0.0))
    same(r["q"], g["q"])
    same(r0["q"], g["q_noU"])
    assert (r0["q_san"] == -50.0).all()
    # what the case is there for
    E0 = len(skeleton.MHR70_15_EDGES)
    assert np.isnan(g["q_med"][[5, E0 + 2, E0 + 3]]).all() and np.isfinite(np.delete(g["q_med"], [5, E0 + 2, E0 + 3])).all()
    assert (g["q_bone"][:, gc.Q_LONE] == -100.0).all() and (g["q_bone"][:, gc.Q_NEVER] == -1e9).all()
    assert g["q_san"][0, 0] == 0.0 and (g["q_san"][[1, 2, 3, 4, 5], [1, 2, 3, 4, 5]] == -50.0).all() and (g["q_san"][:, 7] == -50.0).all()
    assert g["q_temp"][7, 2] == 0.0 and g["q_temp"][8, 2] < 0.0


def test_quality_host_parts():
    c = gc.quality_golden_case()
    g = gc.golden()
    X, med = c["X"], g["q_med"]
    for t in (0, 3, 5):
        same(fuse.q_from_bone_deviation(X[t], c["edges"], med), g["q_bone"][t], sentinels=(-1e9, -100.0))
        same(fuse.q_from_temporal(X[t - 1] if t else None, X[t], beta=c["beta_temp"]), g["q_temp"][t], sentinels=(-1e9,))
        same(fuse.q_2d_sanity(c["U"][t], c["width"], c["height"]), g["q_san"][t], sentinels=(-50.0,))
    same(fuse.combine_q(g["q_bone"], g["q_temp"], g["q_san"], c["w_bone"], c["w_temp"], c["w_san"]), g["q"])
    assert np.isnan(fuse.bone_median_lengths(np.zeros((0, 15, 3)), c["edges"])).all()
    assert (fuse.q_2d_sanity(None, c["width"], c["height"], J=15) == -50.0).all()
    with pytest.raises(ValueError):
        fuse.q_2d_sanity(None, c["width"], c["height"])
    # the bias is added last
    b = g["side_bias"]
    r = fuse.compute_q_nogt(X, c["U"], edges=c["edges"], width=c["width"], height=c["height"], bias=b, med_lens=med)
    assert gc.bits_equal(r["q"], fuse.compute_q_nogt(X, c["U"], edges=c["edges"], width=c["width"], height=c["height"], med_lens=med)["q"] + b)


def test_body_side_bias():
    g = gc.golden()
    names = dict(zip(skeleton.MHR70_15_IDS, skeleton.MHR70_15_NAMES))
    assert np.array_equal(fuse.body_side_bias(skeleton.MHR70_15_IDS, names, 0.75), g["side_bias"])
    assert np.array_equal(fuse.body_side_bias(skeleton.MHR70_15_NAMES, bias_val=0.75), g["side_bias"])
    assert fuse.body_side_bias(skeleton.COCO_NAMES).tolist() == [0] + [1, -1] * 8


def test_group_host_matches_reference():
    g, c = gc.golden(), gc.group_golden_case()
    kw = dict(**gc.KEYS15, sigma_px=c["sigma_px"], sigma_3d=c["sigma_3d"])
    h = gc.host_group(c["X"], c["U"], kw, align=False)
    assert h["pairs"].tolist() == [[0, 1], [0, 2], [1, 2]] and h["fit_ok"].all()
    same(h["fused"], g["g_fused"])
    for p in range(3):
        same(fuse.temporal_smooth_ema(h["fused"][p], gc.IDS15, **c["ema"]), g["g_smoothed"][p])
    assert (h["conf_x"][[0, 2], 4] == 0.0).all() and (h["conf_x"][1, 4] > 0.0).all()      # view 1's key joint is missing in frame 4


@pytest.mark.parametrize("name", sorted(gc.skeleton_golden_inputs()))
def test_skeleton_host_matches_reference(name):
    g = gc.golden()
    for variant in gc.skeleton_variants(name):
        same(gc.host_skeleton(name, variant), g[f"sk_{name}_{variant}"])
    if name.startswith("h36m"):
        X = gc.skeleton_golden_inputs()[name]
        assert gc.bits_equal(skeleton.h36m_to_coco(X, face_mode="approx"), gc.host_skeleton(name, "coco_face"))
        assert np.isnan(gc.host_skeleton(name, "coco")[..., 1:5, :]).all()


def test_skeleton_degenerate_branch_is_taken():
    g = gc.golden()
    deg, normal = g["sk_h36m3_deg_coco_face"], g["sk_h36m3_coco_face"]
    head = g["sk_h36m3_deg"][:, skeleton.H36M["HEAD"]]
    side = deg[:, skeleton.COCO["L_EYE"]] - deg[:, skeleton.COCO["R_EYE"]]
    assert np.allclose(side, [[0.5, 0.0, 0.0]] * 4, atol=1e-8) and np.isfinite(normal[:, 1:5]).all()      # 2 * 0.25 * ||(1, 0, 0)||
    assert np.allclose(0.5 * (deg[:, 1] + deg[:, 2]) - head, 0.5 * (deg[:, 3] + deg[:, 4]) - head + (0.10 - 0.15) * (
        (head - g["sk_h36m3_deg"][:, 9]) / np.linalg.norm(head - g["sk_h36m3_deg"][:, 9], axis=1, keepdims=True)), atol=1e-8)
    # a NaN clip mean takes the normal branch: the frames without the NaN get eyes
    assert np.isfinite(g["sk_h36m3_nan_coco_face"][[0, 2], 1:5]).all() and np.isnan(g["sk_h36m3_nan_coco_face"][[1, 3], 1:5]).any()


def test_skeleton_round_trip_and_refusals():
    X = gc.skeleton_golden_inputs()["coco3"]
    back = skeleton.h36m_to_coco(skeleton.coco_to_h36m(X))
    assert gc.bits_equal(back[:, skeleton.COCO_LIMB_IDX], X[:, skeleton.COCO_LIMB_IDX])
    for bad in (np.zeros((16, 3)), np.zeros((2, 15, 3)), np.zeros((17, 4)), np.zeros(17), np.zeros((1, 2, 17, 3))):
        with pytest.raises(ValueError):
            skeleton.coco_to_h36m(bad)
        with pytest.raises(ValueError):
            skeleton.h36m_to_coco(bad)
    assert skeleton.coco_to_h36m(np.zeros((0, 17, 3))).shape == (0, 17, 3)
    assert skeleton.h36m_to_coco(np.zeros((0, 17, 2)), synthesize_face=True).shape == (0, 17, 2)


# ---- run.fuse_camera_group: the host-only parts --------------------------------------------------------------------------
def _fake_layer(calls):
    """geometry's two calls on CPU tensors, through the host functions"""
    def fuse_group(X, U, *, align, quality, **kw):
        calls.append(("fuse_group", tuple(X.shape)))
        h = gc.host_group(X.numpy(), U.numpy(), kw, align=align)
        return types.SimpleNamespace(pairs=torch.from_numpy(h["pairs"]), fused=torch.from_numpy(h["fused"]))

    def smooth_ema(X, target_ids=None, **kw):
        calls.append(("smooth_ema", tuple(X.shape)))
        return types.SimpleNamespace(X=torch.from_numpy(np.stack([fuse.temporal_smooth_ema(x, target_ids, **kw) for x in X.numpy()])))

    return types.SimpleNamespace(fuse_group=fuse_group, smooth_ema=smooth_ema)


def test_fuse_camera_group_host_parts(tmp_path):
    g, c = gc.golden(), gc.group_golden_case()
    X, U = c["X"], c["U"]
    paths = [tmp_path / "in" / n for n in ("front_sam_3d_body_outputs.npz", "side_outputs.npz", "back.npz")]
    paths[0].parent.mkdir()
    extra = np.concatenate([X[1], X[1][:2]]), np.concatenate([U[1], U[1][:2]])           # a longer sequence: cut to the shortest
    gc.write_camera_npz(paths[0], U[0], X[0])
    gc.write_camera_npz(paths[1], extra[1], extra[0])
    gc.write_camera_npz(paths[2], U[2], X[2], key="frames")                                 # no `outputs` key: the first key
    assert [run.camera_name_from_path(p) for p in paths] == ["front", "side", "back"]
    assert run.camera_name_from_path("a/b/cam_outputs_sam_3d_body_output.npz") == "cam_outputs"
    names, Uh, Xh = run.group_inputs(paths)
    assert names == ["front", "side", "back"] and gc.bits_equal(Xh, X) and gc.bits_equal(Uh, U)
    calls = []
    fuse_kw = dict(**gc.KEYS15, sigma_px=c["sigma_px"], sigma_3d=c["sigma_3d"], scale_mode="hip", min_points=8, align=False)

    def fake(inputs, out_dir, names=None, save_raw_fused=False):
        """run.fuse_camera_group's body on the host: the fake layer, CPU tensors"""
        return run._fuse_camera_group(_fake_layer(calls), torch.device("cpu"), inputs, out_dir, names, None, fuse_kw, c["ema"],
                                      "confidence", None, None, save_raw_fused)

    out = tmp_path / "out"
    r = fake(paths, out)
    assert calls == [("fuse_group", (3, 6, 15, 3)), ("smooth_ema", (3, 6, 15, 3))]              # one call each
    assert sorted(p.name for p in out.iterdir()) == ["front__back_smoothed.npy", "front__side_smoothed.npy", "side__back_smoothed.npy"]
    for p, stem in enumerate(("front__side", "front__back", "side__back")):
        arr = np.load(out / f"{stem}_smoothed.npy")
        assert arr.dtype == np.float64 and arr.shape == (6, 15, 3)
        same(arr, g["g_smoothed"][p])
    assert np.isnan(g["g_smoothed"]).any()
    r = fake([(U[v], X[v]) for v in range(3)], tmp_path / "out2", names=["a", "b", "c"], save_raw_fused=True)
    assert sorted(p.name for p in (tmp_path / "out2").iterdir()) == sorted(f"{s}_{k}.npy" for s in ("a__b", "a__c", "b__c")
                                                                           for k in ("fused", "smoothed"))
    same(np.load(tmp_path / "out2" / "a__c_fused.npy"), g["g_fused"][1])
    assert len(r["paths"]) == 6 and r["pairs"].tolist() == [[0, 1], [0, 2], [1, 2]]
    with pytest.raises(ValueError):
        fake(paths[:1], out)
    with pytest.raises(ValueError):
        fake([(U[0][:0], X[0][:0]), (U[1], X[1])], out)


# ---- the C entry points refuse bad arguments before any launch -------------------------------------------------------------
def test_entry_points_refuse_bad_arguments():
    from skiing_analysis_pytorch_amd import _lib
    lib = _lib.lib()
    assert lib.skimi_fuse_group_workspace_bytes(8, 243, 15) == 8 * 243 * 15 * 3 * 8
    assert lib.skimi_fuse_group_workspace_bytes(8, 243, 129) == 0
    none = [None] * 9
    assert lib.skimi_joint_quality(None, None, 1, 4, 0, None, 0, None, 1.0, 1.0, 0.3, 0.2, 0, None, 0, None, None, None, None, None, None) != 0
    assert b"joints = 0" in lib.skimi_last_error()
    assert lib.skimi_joint_quality(None, None, 1, 4, 15, None, 0, None, 1.0, 1.0, 0.3, 0.2, 0, None, 7, None, None, None, None, None, None) != 0
    assert b"bias_stride" in lib.skimi_last_error()
    assert lib.skimi_joint_quality(None, None, 1, 4, 15, None, 0, None, 1.0, 1.0, 0.3, 0.2, 0, None, 0, None, None, None, None, None, None) != 0
    assert b"NULL" in lib.skimi_last_error()
    assert lib.skimi_joint_quality(None, None, 0, 4, 15, None, 0, None, 1.0, 1.0, 0.3, 0.2, 0, None, 0, None, None, None, None, None, None) == 0
    assert lib.skimi_fuse_group(None, None, None, 3, 4, 15, 14, 11, 12, 5, 15, 12.0, 0.08, 0, 8, 0, None, 0, *none, None) != 0
    assert b"key joint 4" in lib.skimi_last_error()
    assert lib.skimi_fuse_group(None, None, None, 3, 4, 15, 14, 11, 12, 5, 6, 12.0, 0.08, 2, 8, 0, None, 0, *none, None) != 0
    assert b"scale_mode" in lib.skimi_last_error()
    assert lib.skimi_fuse_group(None, None, None, 3, 0, 15, 14, 11, 12, 5, 6, 12.0, 0.08, 0, 8, 0, None, 0, *none, None) == 0
    assert lib.skimi_smooth_ema_batch(None, 0, 5, 15, None, 1, 0.45, 0.92, 0.25, None, None) == 0
    assert lib.skimi_smooth_ema_batch(None, 2, 5, 15, None, 1, 0.45, 0.92, 0.25, None, None) != 0
    assert lib.skimi_convert_skeleton(None, 3, 4, 0, 1, None, None) != 0 and b"coords" in lib.skimi_last_error()
    assert lib.skimi_convert_skeleton(None, 3, 3, 2, 1, None, None) != 0 and b"direction" in lib.skimi_last_error()
    assert lib.skimi_convert_skeleton(None, 0, 3, 1, 1, None, None) == 0
    # the synthesized face sums the clip mean in every workgroup: limited to 2^20 frames, the other forms to 2^34
    assert lib.skimi_convert_skeleton(None, 2 ** 20 + 1, 3, 1, 1, None, None) != 0 and b"2^20" in lib.skimi_last_error()
    assert lib.skimi_convert_skeleton(None, 2 ** 20 + 1, 3, 1, 0, None, None) != 0 and b"NULL" in lib.skimi_last_error()
