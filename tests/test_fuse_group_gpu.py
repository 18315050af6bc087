"""GPU: the joint quality, the group fusion, the batched EMA (csrc/fuse.hip: skimi_joint_quality, skimi_fuse_group,
skimi_smooth_ema_batch) and the skeleton conversion (csrc/skeleton.hip: skimi_convert_skeleton) against the host functions
of skiing_analysis_pytorch_amd/fuse.py and skeleton.py on the same float64 inputs (tests/fuse_group_cases.py; pinned to
the reference by tests/test_fuse_group_cpu.py).  NaN patterns, sentinels, fit_ok and pairs must be equal and every float
within 1e-9 (1 + |x|), the project's float64 tolerance (medians included: the host's norm may round its last bit
differently); bitwise checks are device against device.  Then the wiring: angle.analyze(layout=COCO_17),
infer.process_multi_view_clip(skeleton="h36m") and run.fuse_camera_group."""
import itertools
import json

import numpy as np
import pytest
import torch

import fuse_cases as fc
import fuse_group_cases as gc
from skiing_analysis_pytorch_amd import _lib, angle, fuse, geometry, infer, run, skeleton, vggt, weights as W
from skiing_analysis_pytorch_amd._lib import PREC_BF16X3

pytestmark = pytest.mark.gpu
TOL = gc.TOL
Q_FIELDS = ("q", "q_bone", "q_temp", "q_san")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def quality_call(c, U=True, **kw):
    return geometry.joint_quality(dev(c["X"]), dev(c["U"]) if U else None, edges=c["edges"], size=gc.QUALITY_SIZE,
                                  **{**gc.QUALITY_KW, **kw})


def check_quality(r, h, label):
    for s, k in ((-1e9, "q_bone"), (-100.0, "q_bone"), (-1e9, "q_temp"), (0.0, "q_temp"), (-50.0, "q_san"), (0.0, "q_san")):
        assert np.array_equal(host(getattr(r, k)) == s, h[k] == s), f"{label}: {k} places {s} differently"
    worst = {k: fc.close(host(getattr(r, k)), h[k], TOL) for k in Q_FIELDS + ("med_lens",)}
    print(f"joint_quality {label}: worst |dev - host| / (1 + |host|): " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))


# ---- joint quality ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", gc.QUALITY_T)
def test_joint_quality_matches_host_over_T(T):
    c, h = gc.quality_case(T, 15), gc.host_quality_case(T, 15)
    r = quality_call(c)
    assert r.q.shape == (1, T, 15) and r.med_lens.shape == (1, len(c["edges"])) and r.q.is_cuda
    check_quality(r, h, f"T={T}")
    if T == 0:
        assert bool(torch.isnan(r.med_lens).all())


@pytest.mark.parametrize("J", gc.QUALITY_J)
def test_joint_quality_matches_host_over_J(J):
    c, h = gc.quality_case(6, J, 2), gc.host_quality_case(6, J, 2)
    check_quality(quality_call(c), h, f"J={J}")
    assert (h["q_bone"][:, :, J - 1][np.isfinite(c["X"][:, :, J - 1]).all(-1)] == -100.0).all()      # the joint without an edge
    assert (h["q_bone"][:, :, 3] == -1e9).all() and np.isnan(h["med_lens"][:, [2, 3]]).all()          # the joint never seen


def test_joint_quality_matches_reference_clip():
    g, c = gc.golden(), gc.quality_golden_case()
    kw = dict(edges=c["edges"], size=(c["width"], c["height"]), beta_temp=c["beta_temp"], w_bone=c["w_bone"], w_temp=c["w_temp"],
              w_san=c["w_san"])
    r = geometry.joint_quality(dev(c["X"]), dev(c["U"]), **kw)                       # [T, J, 3]: V = 1, no view axis in the results
    assert r.q.shape == (9, 15) and r.med_lens.shape == (len(c["edges"]),)
    for k, name in (("q", "q"), ("q_bone", "q_bone"), ("q_temp", "q_temp"), ("q_san", "q_san"), ("med_lens", "q_med")):
        fc.close(host(getattr(r, k)), g[name], TOL)
    assert np.array_equal(host(r.q_bone) == -100.0, g["q_bone"] == -100.0) and np.array_equal(host(r.q_bone) == -1e9, g["q_bone"] == -1e9)
    r0 = geometry.joint_quality(dev(c["X"]), None, **kw)
    fc.close(host(r0.q), g["q_noU"], TOL)
    assert bool((r0.q_san == -50.0).all())


def test_joint_quality_no_edges_no_U_bias_and_sizes():
    c = gc.quality_case(5, 17, 3)
    X, U = c["X"], c["U"]
    r = geometry.joint_quality(dev(X), None, edges=[], size=gc.QUALITY_SIZE, **gc.QUALITY_KW)
    h = gc.host_quality(X, None, [], **gc.QUALITY_KW)
    assert r.med_lens.shape == (3, 0)
    one = geometry.joint_quality(dev(X[0]), None, edges=[], size=gc.QUALITY_SIZE, med_lens=np.zeros(0), **gc.QUALITY_KW)
    assert one.med_lens.shape == (0,) and same_bits(one.q, r.q[0])                  # [T, J, 3] with given medians and E = 0
    check_quality(r, h, "E=0, U=None")
    assert set(np.unique(host(r.q_bone))) <= {-1e9, -100.0} and bool((r.q_san == -50.0).all())
    # one size and one bias per view
    rng = np.random.default_rng(5)
    size, bias = np.array([[640.0, 360.0], [100.0, 700.0], [641.0, 1.0]]), rng.normal(size=(3, 17))
    r = geometry.joint_quality(dev(X), dev(U), edges=c["edges"], size=size, bias=dev(bias), **gc.QUALITY_KW)
    check_quality(r, gc.host_quality(X, U, c["edges"], size=size, bias=bias, **gc.QUALITY_KW), "per-view size and bias")
    plain = quality_call(c)
    assert same_bits(geometry.joint_quality(dev(X), dev(U), edges=c["edges"], size=gc.QUALITY_SIZE, bias=bias[0], **gc.QUALITY_KW).q,
                     plain.q + dev(bias[0]))


def test_joint_quality_given_medians_make_a_frame_independent_of_its_clip():
    c = gc.quality_case(67, 17)
    X, U = c["X"], c["U"]
    med = dev(gc.host_quality_case(67, 17)["med_lens"])
    full = quality_call(c, med_lens=med)
    assert same_bits(full.med_lens, med)
    check_quality(full, gc.host_quality(X, U, c["edges"], med_lens=host(med), **gc.QUALITY_KW), "med_lens given")
    # frames 40, 41 moved to the front of another clip: frame 41 keeps every bit, frame 40 all but its q_temp
    other = gc.quality_case(5, 17)
    X2, U2 = np.concatenate([X[:, 40:42], other["X"]], axis=1), np.concatenate([U[:, 40:42], other["U"]], axis=1)
    moved = geometry.joint_quality(dev(X2), dev(U2), edges=c["edges"], size=gc.QUALITY_SIZE, med_lens=med, **gc.QUALITY_KW)
    for k in Q_FIELDS:
        assert same_bits(getattr(moved, k)[:, 1], getattr(full, k)[:, 41]), k
    for k in ("q_bone", "q_san"):
        assert same_bits(getattr(moved, k)[:, 0], getattr(full, k)[:, 40]), k


def test_joint_quality_views_are_independent_and_runs_reproducible():
    c = gc.quality_case(130, 65, 3)
    r, again = quality_call(c), quality_call(c)
    for k in Q_FIELDS + ("med_lens",):
        assert same_bits(getattr(r, k), getattr(again, k)), k
    for v in range(3):
        one = geometry.joint_quality(dev(c["X"][v]), dev(c["U"][v]), edges=c["edges"], size=gc.QUALITY_SIZE, **gc.QUALITY_KW)
        for k in Q_FIELDS + ("med_lens",):
            assert same_bits(getattr(one, k), getattr(r, k)[v]), (k, v)
    check_quality(r, gc.host_quality_case(130, 65, 3), "T=130, J=65, V=3")


def test_joint_quality_refuses_bad_arguments():
    c = gc.quality_case(2, 15)
    X, U = dev(c["X"]), dev(c["U"])
    with pytest.raises(_lib.SkimiError):
        geometry.joint_quality(torch.zeros(2, 15, 3), edges=[], size=gc.QUALITY_SIZE)
    for bad in (dict(U=U[:, :1]), dict(size=(1.0, 2.0, 3.0)), dict(bias=np.zeros(14)), dict(med_lens=np.zeros((1, 3))), dict(edges=[(0, 1, 2)])):
        kw = dict(U=U, edges=c["edges"], size=gc.QUALITY_SIZE) | bad
        with pytest.raises(ValueError):
            geometry.joint_quality(X, kw.pop("U"), **kw)
    with pytest.raises(_lib.SkimiError):
        geometry.joint_quality(torch.zeros(1, 2, 129, 3, dtype=torch.float64, device="cuda"), edges=[], size=gc.QUALITY_SIZE)


# ---- group fusion -----------------------------------------------------------------------------------------------------
VIEW_OF_PAIR = (("fused", "fused"), ("aligned", "aligned"), ("q_a", "q_l"), ("q_b", "q_r"), ("conf_x", "conf_x"), ("dist", "dist"))


def group_call(c, **kw):
    return geometry.fuse_group(dev(c["X"]), dev(c["U"]), **{**c["kw"], **kw})


@pytest.mark.parametrize("V", (1, 2, 3, 5))
def test_fuse_group_pairs_and_agreement_with_fuse_views(V):
    c = gc.group_case(V)
    X, U = dev(c["X"]), dev(c["U"])
    r = group_call(c, align=True)
    pairs = list(itertools.combinations(range(V), 2))
    assert r.pairs.dtype == torch.int32 and host(r.pairs).reshape(-1, 2).tolist() == [list(p) for p in pairs]
    assert r.fused.shape == (len(pairs), 5, 70, 3) and r.conf.shape == (V, 5, 70) and r.fit_ok.shape == (V, 5) and r.fit_ok.dtype == torch.bool
    for p, (a, b) in enumerate(pairs):
        w = geometry.fuse_views(X[a], X[b], U[a], U[b], **c["kw"])
        for mine, theirs in VIEW_OF_PAIR:
            assert same_bits(getattr(r, mine)[p], getattr(w, theirs)), (a, b, mine)
        assert same_bits(r.conf[a], w.conf_l) and same_bits(r.conf[b], w.conf_r) and same_bits(r.err[a], w.err_l) and same_bits(r.err[b], w.err_r)
        assert torch.equal(r.fit_ok[a], w.fit_ok[:, 0]) and torch.equal(r.fit_ok[b], w.fit_ok[:, 1])
    conf, err, ok = gc.host_view_conf(c["X"], c["U"], c["kw"])
    assert np.array_equal(host(r.fit_ok), ok) and not ok[0, 3] and not ok[V - 1, 4]
    fc.close(host(r.conf), conf, TOL)
    fc.close(host(r.err), err, TOL)


def test_fuse_group_agrees_with_fuse_views_on_its_own_clip():
    """the two-view clip of tests/fuse_cases.py (missing key joints, fewer than min_points rows, fewer than 3 common joints)
    plus a third view made from its right one"""
    c = fc.views_cases()["J70_T65_mixed"]
    X = np.stack([c["Xl"], c["Xr"], 0.97 * (c["Xr"] @ fc._rot_y(-0.4).T) + 0.05])
    U = np.stack([c["Ul"], c["Ur"], c["Ur"][::-1].copy()])
    r = geometry.fuse_group(dev(X), dev(U), align=True, **c["kw"])
    w = geometry.fuse_views(*(dev(c[k]) for k in ("Xl", "Xr", "Ul", "Ur")), **c["kw"])
    for mine, theirs in VIEW_OF_PAIR:
        assert same_bits(getattr(r, mine)[0], getattr(w, theirs)), mine
    assert torch.equal(r.fit_ok[:2].T, w.fit_ok)
    h = fc.host_views_case("J70_T65_mixed")
    for mine, theirs in VIEW_OF_PAIR:
        fc.close(host(getattr(r, mine)[0]), h[theirs], TOL)


def test_fuse_group_unaligned_matches_reference_and_host():
    g, c = gc.golden(), gc.group_golden_case()
    kw = dict(**gc.KEYS15, sigma_px=c["sigma_px"], sigma_3d=c["sigma_3d"])
    r = geometry.fuse_group(dev(c["X"]), dev(c["U"]), align=False, **kw)
    fc.close(host(r.fused), g["g_fused"], TOL)
    for p, (a, b) in enumerate(gc.pairs_of(3)):
        assert same_bits(r.aligned[p], dev(c["X"][b]))
    h = gc.host_group(c["X"], c["U"], kw, align=False)
    worst = {k: fc.close(host(getattr(r, k)), h[k], TOL) for k in ("fused", "q_a", "q_b", "conf_x", "dist", "conf", "err")}
    print("fuse_group align=False: worst |dev - host| / (1 + |host|): " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    sm = geometry.smooth_ema(r.fused, target_ids=gc.IDS15, **c["ema"])
    fc.close(host(sm.X), g["g_smoothed"], TOL)
    # the larger clip with frames where the host raises, both alignments
    c = gc.group_case(3)
    for align in (False, True):
        r, h = group_call(c, align=align), gc.host_group(c["X"], c["U"], c["kw"], align=align)
        for k in ("fused", "aligned", "q_a", "q_b", "conf_x", "dist", "conf", "err"):
            fc.close(host(getattr(r, k)), h[k], TOL)
        assert np.array_equal(host(r.fit_ok), h["fit_ok"])


def test_fuse_group_given_qualities():
    c = gc.group_case(3)
    X, U = c["X"], c["U"]
    edges = [(j, j + 1) for j in range(69)]
    q = geometry.joint_quality(dev(X), dev(U), edges=edges, size=(1280.0, 720.0)).q
    for align in (False, True):
        r = geometry.fuse_group(dev(X), None, quality=q, align=align, **c["kw"])
        assert r.conf_x is None and r.dist is None and r.conf is None and r.err is None and r.fit_ok is None
        h = gc.host_group(X, U, c["kw"], align=align, quality=host(q))
        for k in ("fused", "aligned"):
            fc.close(host(getattr(r, k)), h[k], TOL)
        for p, (a, b) in enumerate(gc.pairs_of(3)):
            assert same_bits(r.q_a[p], q[a]) and same_bits(r.q_b[p], q[b])
    assert same_bits(geometry.fuse_group(dev(X), dev(U), quality=q, align=True, **c["kw"]).fused, r.fused)       # U is not read
    with pytest.raises(ValueError):
        geometry.fuse_group(dev(X), None, quality=q[:2], **c["kw"])
    with pytest.raises(ValueError):
        geometry.fuse_group(dev(X), dev(U), quality="nogt", **c["kw"])
    with pytest.raises(_lib.SkimiError):
        geometry.fuse_group(dev(X), None, **c["kw"])


def test_fuse_group_pairs_are_independent_and_runs_reproducible():
    c = gc.group_case(5)
    X, U = dev(c["X"]), dev(c["U"])
    r, again = group_call(c), group_call(c)
    fields = ("fused", "aligned", "q_a", "q_b", "conf_x", "dist")
    for k in fields + ("conf", "err"):
        assert same_bits(getattr(r, k), getattr(again, k)), k
    pairs = gc.pairs_of(5)
    sub = [0, 2, 4]
    rs = geometry.fuse_group(X[sub].contiguous(), U[sub].contiguous(), **c["kw"])
    for p, (a, b) in enumerate(gc.pairs_of(3)):
        full = pairs.index((sub[a], sub[b]))
        for k in fields:
            assert same_bits(getattr(rs, k)[p], getattr(r, k)[full]), (k, a, b)
    e = geometry.fuse_group(X[:, :0].contiguous(), U[:, :0].contiguous(), **c["kw"])
    assert e.fused.shape == (10, 0, 70, 3) and e.fit_ok.shape == (5, 0) and host(e.pairs).tolist() == [list(p) for p in pairs]


# ---- batched EMA ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", (1, 3))
@pytest.mark.parametrize("variant", range(len(fc.EMA_VARIANTS)))
def test_smooth_ema_batch_equals_single_calls(B, variant):
    clips = [fc.smooth_clip(9)] + [np.roll(fc.smooth_clip(9), k, axis=1) * (1.0 + 0.1 * k) for k in range(1, B)]
    X = dev(np.stack(clips))
    kw = fc.ema_kw(9, variant)
    r = geometry.smooth_ema(X, **kw)
    assert r.X.shape == X.shape
    for b in range(B):
        one = geometry.smooth_ema(X[b], **kw)
        assert same_bits(r.X[b], one.X) and same_bits(r.base, one.base)
    fc.close(host(r.X[0]), fc.host_ema(9, variant), TOL)


def test_smooth_ema_batch_empty_and_long():
    e = geometry.smooth_ema(torch.empty((0, 4, 6, 3), dtype=torch.float64, device="cuda"))
    assert e.X.shape == (0, 4, 6, 3)
    X = dev(np.stack([fc.smooth_clip(500), fc.smooth_clip(500)[::-1].copy()]))
    r = geometry.smooth_ema(X)
    assert same_bits(r.X[1], geometry.smooth_ema(X[1]).X)
    fc.close(host(r.X[0]), fc.host_ema(500, 0), TOL)
    with pytest.raises(ValueError):
        geometry.smooth_ema(torch.zeros((2, 4, 6, 2), dtype=torch.float64, device="cuda"))


# ---- skeleton conversion ----------------------------------------------------------------------------------------------
def skeleton_call(name, variant):
    X = gc.skeleton_golden_inputs()[name]
    if variant.startswith("h36m"):
        return geometry.convert_skeleton(dev(X), "coco_to_h36m", synthesize_head=variant == "h36m")
    return geometry.convert_skeleton(dev(X), "h36m_to_coco", synthesize_face=variant == "coco_face")


@pytest.mark.parametrize("name", sorted(gc.skeleton_golden_inputs()))
def test_convert_skeleton_matches_reference_and_host(name):
    g = gc.golden()
    for variant in gc.skeleton_variants(name):
        r = skeleton_call(name, variant)
        assert r.is_cuda and r.dtype == torch.float64 and r.shape == gc.skeleton_golden_inputs()[name].shape
        fc.close(host(r), g[f"sk_{name}_{variant}"], TOL)
        fc.close(host(r), gc.host_skeleton(name, variant), TOL)
        assert same_bits(r, skeleton_call(name, variant))


def test_convert_skeleton_round_trip_host_arrays_and_refusals():
    X = gc.skeleton_golden_inputs()["coco3"]
    h = geometry.convert_skeleton(X, "coco_to_h36m")                                  # a host array is uploaded
    assert h.is_cuda and same_bits(h, geometry.convert_skeleton(dev(X), "coco_to_h36m"))
    back = geometry.convert_skeleton(h, "h36m_to_coco")
    assert same_bits(back[:, skeleton.COCO_LIMB_IDX], dev(X)[:, skeleton.COCO_LIMB_IDX])
    assert same_bits(skeleton.coco_to_h36m(dev(X)), h) and same_bits(skeleton.h36m_to_coco(h), back)       # the host module's names
    assert same_bits(geometry.convert_skeleton(dev(X.astype(np.float32)), "coco_to_h36m"),
                     geometry.convert_skeleton(dev(X.astype(np.float32).astype(np.float64)), "coco_to_h36m"))
    # more than one workgroup of frames: the clip mean is the same in each
    big = np.tile(gc.skeleton_golden_inputs()["h36m3"], (150, 1, 1))
    fc.close(host(geometry.convert_skeleton(dev(big), "h36m_to_coco", synthesize_face=True)), skeleton.h36m_to_coco(big, synthesize_face=True), TOL)
    deg = np.tile(gc.skeleton_golden_inputs()["h36m3_deg"], (150, 1, 1))
    fc.close(host(geometry.convert_skeleton(dev(deg), "h36m_to_coco", synthesize_face=True)), skeleton.h36m_to_coco(deg, synthesize_face=True), TOL)
    assert geometry.convert_skeleton(dev(np.zeros((0, 17, 3))), "h36m_to_coco", synthesize_face=True).shape == (0, 17, 3)
    for bad in (np.zeros((16, 3)), np.zeros((2, 15, 3)), np.zeros((17, 4)), np.zeros((1, 2, 17, 3))):
        with pytest.raises(ValueError):
            geometry.convert_skeleton(dev(bad), "coco_to_h36m")
    with pytest.raises(ValueError):
        geometry.convert_skeleton(dev(X), "coco_to_smpl")
    with pytest.raises(_lib.SkimiError):
        geometry.convert_skeleton(torch.zeros(17, 3), "coco_to_h36m")


# ---- wiring -----------------------------------------------------------------------------------------------------------
def _coco_clip(T=40):
    rng = np.random.default_rng(61)
    h = fc._walk(rng, fc._H36M_BODY, T, amp=0.06)
    return skeleton.h36m_to_coco(h, synthesize_face=True)


def test_angle_analyze_takes_coco17():
    coco = _coco_clip()
    a = angle.analyze(coco, layout=angle.COCO_17)
    b = angle.analyze(geometry.convert_skeleton(coco, "coco_to_h36m"), layout=angle.H36M_17)
    assert a.series.keys() == b.series.keys() and all(gc.bits_equal(a.series[k], b.series[k]) for k in a.series)
    assert gc.bits_equal(a.heading, b.heading) and a.turns == b.turns and gc.bits_equal(a.stats, b.stats)
    assert np.isfinite(a.series["knee_l"]).all()
    joint, *_ = angle.compute_all_series(coco, layout=angle.COCO_17)
    assert gc.bits_equal(joint["knee_l"], a.series["knee_l"])
    with pytest.raises(ValueError):
        angle.analyze(coco[:, :15], layout=angle.COCO_17)


def test_angle_process_person_pair_takes_coco17(tmp_path):
    coco = _coco_clip()
    h36m = skeleton.coco_to_h36m(coco)
    for name, arr in (("s_coco", coco), ("f_coco", coco[:30]), ("s_h36m", h36m), ("f_h36m", h36m[:30])):
        np.save(tmp_path / f"{name}.npy", arr)
    a = angle.process_person_pair(tmp_path / "s_coco.npy", tmp_path / "f_coco.npy", tmp_path / "coco", layout=angle.COCO_17)
    b = angle.process_person_pair(tmp_path / "s_h36m.npy", tmp_path / "f_h36m.npy", tmp_path / "h36m", layout=angle.H36M_17)
    for x, y in zip(a, b):
        assert all(gc.bits_equal(x.series[k], y.series[k]) for k in x.series) and gc.bits_equal(x.heading, y.heading)
    assert sorted(p.name for p in (tmp_path / "coco").rglob("*.csv")) == sorted(p.name for p in (tmp_path / "h36m").rglob("*.csv"))


def test_clip_path_returns_h36m_joints(golden_dir):
    g = np.load(golden_dir / "vggt_tiny_conv.npz")
    cfg = W.VGGTConfig(**json.loads(str(g["cfg_json"])))
    m = vggt.VGGT(config=cfg, prec=PREC_BF16X3, head_prec=PREC_BF16X3)
    m.load_state_dict(W.make_vggt_state_dict(cfg, seed=0))
    T, S, H, Wd = 2, 2, 140, 140
    frames = torch.stack([W.make_images(S, H, Wd, seed=70 + t) for t in range(T)]).cuda()
    rng = np.random.default_rng(7)
    kps = torch.from_numpy(rng.uniform(20.0, 120.0, size=(T, S, 17, 2)).astype(np.float32)).cuda()
    kw = dict(steps_per_call=2, smooth=True, device_smooth=True)
    plain = infer.process_multi_view_clip(m, frames, kps, **kw)
    out = infer.process_multi_view_clip(m, frames, kps, skeleton="h36m", **kw)
    assert set(out) - set(plain) == {"joints3d_h36m", "joints3d_smoothed_h36m"}
    for k in plain:
        assert same_bits(out[k], plain[k]), k
    for k in ("joints3d", "joints3d_smoothed"):
        r = out[k + "_h36m"]
        assert r.is_cuda and r.dtype == torch.float64 and r.shape == (T, 17, 3)
        assert same_bits(r, geometry.convert_skeleton(plain[k], "coco_to_h36m"))
    host_smooth = infer.process_multi_view_clip(m, frames, kps, skeleton="h36m", steps_per_call=2, smooth=True)
    assert host_smooth["joints3d_smoothed_h36m"].is_cuda and not host_smooth["joints3d_smoothed"].is_cuda
    calls = []
    with pytest.raises(ValueError):
        infer.process_multi_view_clip(lambda *a, **k: calls.append(1), frames, kps[:, :, :15], skeleton="h36m")
    with pytest.raises(ValueError):
        infer.process_multi_view_clip(lambda *a, **k: calls.append(1), frames, kps, skeleton="coco")
    assert not calls


def test_fuse_camera_group_writes_the_reference_files(tmp_path):
    g, c = gc.golden(), gc.group_golden_case()
    X, U = c["X"], c["U"]
    paths = [tmp_path / n for n in ("front_sam_3d_body_outputs.npz", "side_outputs.npz", "back.npz")]
    for v, p in enumerate(paths):
        gc.write_camera_npz(p, U[v], X[v])
    kw = dict(sigma_px=c["sigma_px"], sigma_3d=c["sigma_3d"], alpha=c["ema"]["alpha"], adaptive_smooth=c["ema"]["adaptive"],
              smooth_alpha_min=c["ema"]["alpha_min"], smooth_alpha_max=c["ema"]["alpha_max"], smooth_speed_gain=c["ema"]["speed_gain"])
    out = tmp_path / "out"
    r = run.fuse_camera_group(paths, out, **kw)
    assert sorted(p.name for p in out.iterdir()) == ["front__back_smoothed.npy", "front__side_smoothed.npy", "side__back_smoothed.npy"]
    for p, stem in enumerate(("front__side", "front__back", "side__back")):
        arr = np.load(out / f"{stem}_smoothed.npy")
        assert arr.dtype == np.float64
        fc.close(arr, g["g_smoothed"][p], TOL)
    out2 = tmp_path / "out2"
    r = run.fuse_camera_group(paths, out2, save_raw_fused=True, **kw)
    assert len(list(out2.iterdir())) == 6 and len(r["paths"]) == 6
    fc.close(np.load(out2 / "side__back_fused.npy"), g["g_fused"][2], TOL)
    # the ground-truth-free quality instead of the confidences
    r = run.fuse_camera_group(paths, tmp_path / "out3", quality="nogt", size=(640, 360), **kw)
    q = fuse.compute_q_nogt(X[0], U[0], edges=skeleton.MHR70_15_EDGES, width=640, height=360)["q"]
    q2 = fuse.compute_q_nogt(X[2], U[2], edges=skeleton.MHR70_15_EDGES, width=640, height=360)["q"]
    fc.close(r["fused"][1], np.stack([fuse.fuse_frame_3d(X[0, t], X[2, t], q[t], q2[t]) for t in range(6)]), TOL)
