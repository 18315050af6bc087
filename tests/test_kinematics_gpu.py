"""GPU: the kinematic analysis of clips (csrc/kinematics.hip: skimi_kinematics) against the float64 restatement
(tests/kinematics_restated.py, itself held against the reference's outputs by tests/test_kinematics_cpu.py) on every case of
tests/kinematics_cases.py.  NaN masks, boundary, n_turns, turn_frames, turn_direction and turn_counts must be equal and every
float within 1e-9 (1 + |x|), the project's float64 tolerance.  The one exception is the exactly straight limb: its cosine is
+-1 to a few ulps, and k ulps of difference there move acos by sqrt(2 k 1.1e-16) rad, below 4e-6 degrees for k <= 16, so
that angle (and what is computed from it) is held to 1e-5 degrees.  Results must be bitwise reproducible, a clip's the same
alone and inside a ragged batch with garbage in the padding, and the same in both placements of the per-clip arrays.  Then
the entry points: angle.process_person, angle.process_person_pair and run.process_video_3d(analyze=True)."""
import csv
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import kinematics_cases as kc
import kinematics_restated as kr
from skiing_analysis_pytorch_amd import _lib, angle, geometry, run, weights as W

pytestmark = pytest.mark.gpu
TOL = 1e-9
STRAIGHT_TOL_DEG = 1e-5


def device(case, **over):
    kw = {**kc.params(case), **over}
    r = geometry.kinematics(torch.from_numpy(case["X"]).cuda(), **kw)
    torch.cuda.synchronize()
    return r


def host(r):
    return {k: getattr(r, k).cpu().numpy() for k in kc.FLOAT_FIELDS + kc.EXACT_FIELDS}


def same_bits(a, b):
    return all(torch.equal(x.view(torch.uint8) if x.dtype != torch.bool else x, y.view(torch.uint8) if y.dtype != torch.bool else y)
               for x, y in zip(a, b))


def check(name, got, want, tol=TOL):
    for k in kc.EXACT_FIELDS:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), f"{name}: {k} differs"
    w = {k: kc.worst(got[k], want[k]) for k in kc.FLOAT_FIELDS}
    print(f"{name}: worst |dev - restatement| / (1 + |x|): " + ", ".join(f"{k} {v:.1e}" for k, v in w.items()))
    for k, v in w.items():
        assert v <= tol, f"{name}: {k} off by {v:.3e}"
    return w


@pytest.mark.parametrize("name", list(kc.CASES))
def test_against_restatement(name):
    case = kc.CASES[name]
    r = device(case)
    T = case["X"].shape[-3]
    M = kr.max_turns(T, case.get("min_turn_frames", 12))
    assert r.turn_frames.shape[1:] == (M, 2) and r.turn_stats.shape[1:] == (M, 42, 4) and r.series.shape[1:] == (14, T)
    assert r.boundary.dtype == torch.bool and r.n_turns.dtype == torch.int32 and r.turn_frames.dtype == torch.int32
    check(name, host(r), kc.restated(name))


def test_straight_limb():
    r, want = host(device(kc.straight_case())), kc.restated("straight")
    for k in kc.EXACT_FIELDS:
        assert np.array_equal(r[k], want[k]), k
    # what hangs on the straight knee: knee_l and knee_diff_lr, their changes, and the turn statistics of those six series
    touched = [kr.SERIES.index(n) for n in ("knee_l", "knee_diff_lr", "knee_l_d", "knee_l_abs_d", "knee_diff_lr_d", "knee_diff_lr_abs_d")]
    got_all = np.concatenate([r["series"], r["changes"]], axis=1)
    want_all = np.concatenate([want["series"], want["changes"]], axis=1)
    loose = np.zeros(got_all.shape, dtype=bool)
    loose[:, touched, kc.STRAIGHT_FRAMES[0]:kc.STRAIGHT_FRAMES[-1] + 2] = True
    assert np.array_equal(np.isnan(got_all), np.isnan(want_all))
    err = np.abs(got_all - want_all)
    straight = float(np.nanmax(err[loose]))
    rest = float(np.nanmax((err / (1 + np.abs(want_all)))[~loose]))
    k0 = kr.SERIES.index("knee_l")
    print(f"straight limb: knee_l there {got_all[0, k0, 3:6]} vs {want_all[0, k0, 3:6]}, worst {straight:.2e} deg; elsewhere {rest:.1e}")
    assert straight <= STRAIGHT_TOL_DEG and rest <= TOL
    assert (want_all[0, k0, 3:6] > 179.99).all()
    sel = np.zeros(42, dtype=bool)
    sel[touched] = True
    assert np.array_equal(np.isnan(r["turn_stats"]), np.isnan(want["turn_stats"]))
    assert np.nanmax(np.abs(r["turn_stats"] - want["turn_stats"])[:, :, sel], initial=0.0) <= STRAIGHT_TOL_DEG
    assert kc.worst(r["turn_stats"][:, :, ~sel], want["turn_stats"][:, :, ~sel]) <= TOL
    for k in ("heading", "heading_smooth", "velocity_smooth", "turn_heading_change"):
        assert kc.worst(r[k], want[k]) <= TOL


# ---- bits and placements ----------------------------------------------------------------------------------------------
def test_rerun_is_bitwise():
    case = kc.CASES["g243"]
    assert same_bits(device(case), device(case))


def test_clip_alone_and_in_ragged_batch():
    case = kc.CASES["ragged"]
    batch = device(case)
    for b, n in enumerate(case["lengths"]):
        alone = device(dict(X=case["X"][b, :n]))
        m = alone.turn_frames.shape[1]
        assert int(batch.n_turns[b]) == int(alone.n_turns[0]) <= m
        for k in ("series", "changes", "heading", "heading_smooth", "velocity_smooth", "boundary"):
            assert same_bits([getattr(batch, k)[b, ..., :n].contiguous()], [getattr(alone, k)[0]]), (b, k)
        for k in ("turn_frames", "turn_heading_change", "turn_direction", "turn_stats", "turn_counts"):
            assert same_bits([getattr(batch, k)[b, :m].contiguous()], [getattr(alone, k)[0]]), (b, k)
    # other garbage in the padding, another place in the batch: the same bits
    X = case["X"][::-1].copy()
    lengths = case["lengths"][::-1]
    for b, n in enumerate(lengths):
        X[b, n:] = -7.5
    flipped = device(dict(X=X, lengths=lengths))
    for k in kc.FLOAT_FIELDS + kc.EXACT_FIELDS:
        assert same_bits([getattr(flipped, k).flip(0).contiguous()], [getattr(batch, k)]), k


@pytest.mark.parametrize("name", ["g243", "t1025", "ragged", "t4"])
def test_lds_and_workspace_placements(name):
    case = kc.CASES[name]
    assert case["X"].shape[-3] <= geometry.KIN_LDS_FRAMES
    assert same_bits(device(case), device(case, placement="workspace"))


def test_single_clip_input():
    case = kc.CASES["g64"]
    a = geometry.kinematics(torch.from_numpy(case["X"]).cuda())
    b = geometry.kinematics(torch.from_numpy(case["X"][None]).cuda())
    assert a.series.shape == (1, 14, 64) and same_bits(a, b)


# ---- argument errors and the empty batch ------------------------------------------------------------------------------
def test_argument_errors():
    X = torch.from_numpy(kc.CASES["g64"]["X"]).cuda()
    with pytest.raises(_lib.SkimiError):
        geometry.kinematics(X.cpu())
    bad_layouts = [tuple([15] + list(kr.MHR70_15[1:])), tuple([-2] + list(kr.MHR70_15[1:]))]
    for kw in ([dict(layout=lay) for lay in bad_layouts] +
               [dict(up_axis=(0.0, 0.0, 0.0)), dict(up_axis=(0.0, float("nan"), 0.0)), dict(up_axis=(0.0, float("inf"), 0.0)),
                dict(heading_window=10), dict(heading_window=1), dict(velocity_window=4), dict(velocity_window=1),
                dict(min_turn_frames=0)]):
        with pytest.raises(_lib.SkimiError):
            geometry.kinematics(X, **kw)
    with pytest.raises(ValueError):
        geometry.kinematics(X, layout=kr.MHR70_15[:12])
    with pytest.raises(ValueError):
        geometry.kinematics(X[..., :2])


def _raw(T=20, J=15, null=None, max_turns=None, ws_bytes=None, joints=None):
    """skimi_kinematics on buffers filled with 7 -> (return code, outputs untouched)"""
    B = 2
    f64 = lambda *s: torch.full(s, 7.0, dtype=torch.float64, device="cuda")           # noqa: E731
    i32 = lambda *s: torch.full(s, 7, dtype=torch.int32, device="cuda")               # noqa: E731
    M = geometry.kin_max_turns(T)
    X = f64(B, T, J, 3)
    outs = [f64(B, 42, T), f64(B, T), f64(B, T), f64(B, T), torch.full((B, T), 7, dtype=torch.uint8, device="cuda"), i32(B),
            i32(B, M, 2), f64(B, M), i32(B, M), f64(B, M, 42, 4), i32(B, M, 42)]
    ptrs = [_lib.ptr(o) for o in outs]
    ws = None
    if ws_bytes is not None:
        ws = torch.empty((max(ws_bytes, 8) // 8,), dtype=torch.float64, device="cuda")
    if null == "X":
        X = None
    elif isinstance(null, int):
        ptrs[null] = None
    lay = (C.c_int32 * 13)(*kr.MHR70_15)
    up = (C.c_double * 3)(0.0, -1.0, 0.0)
    rc = _lib.lib().skimi_kinematics(_lib.ptr(X), None, B, T, J if joints is None else joints, None if null == "layout" else lay,
                                     None if null == "up" else up, 12, 8.0, 11, 9, M if max_turns is None else max_turns,
                                     _lib.ptr(ws), ws_bytes or 0, *ptrs, _lib.current_stream())
    torch.cuda.synchronize()
    return rc, all(bool((o == 7).all()) for o in outs)


def test_raw_argument_errors():
    assert _raw()[0] == 0
    for kw in ([dict(null=n) for n in ["X", "layout", "up"] + list(range(11))] +
               [dict(joints=0), dict(joints=14), dict(max_turns=1), dict(T=geometry.KIN_LDS_FRAMES + 1),
                dict(ws_bytes=2 * 3 * 20 * 8 - 8)]):
        rc, untouched = _raw(**kw)
        assert rc != 0 and untouched, kw
    assert _raw(ws_bytes=2 * 3 * 20 * 8)[0] == 0
    assert _lib.lib().skimi_kin_workspace_bytes(2, 20) == 2 * 3 * 20 * 8 and _lib.lib().skimi_kin_workspace_bytes(2, 21) == 2 * 3 * 22 * 8
    assert _lib.lib().skimi_kin_workspace_bytes(-1, 20) == 0 and _lib.lib().skimi_kin_workspace_bytes(2, 0) == 0


def test_empty_batch_and_empty_clips():
    r = geometry.kinematics(torch.zeros((0, 30, 15, 3), dtype=torch.float64, device="cuda"))
    assert r.series.shape == (0, 14, 30) and r.n_turns.shape == (0,) and r.turn_stats.shape == (0, 3, 42, 4)
    r = geometry.kinematics(torch.zeros((2, 0, 15, 3), dtype=torch.float64, device="cuda"))
    assert r.series.shape == (2, 14, 0) and r.turn_frames.shape == (2, 0, 2) and r.n_turns.tolist() == [0, 0]
    r = geometry.kinematics(torch.from_numpy(kc.CASES["g64"]["X"][None].repeat(2, 0)).cuda(), lengths=[0, 64])
    assert r.n_turns.tolist() == [0, 3] and bool(torch.isnan(r.series[0]).all()) and not bool(r.boundary[0].any())


# ---- entry points -----------------------------------------------------------------------------------------------------
def _read(path):
    with open(path, newline="") as f:
        rows = list(csv.reader(f))
    return rows[0], rows[1:]


def _check_person(out, want, T):
    """the CSVs of process_person under `out` against a restated result (one clip)"""
    full, turn = out / "non_turn_evaluation", out / "turn_evaluation"
    every = np.concatenate([want["series"][0], want["changes"][0]])
    for fname, names in angle.SERIES_FILES.items():
        head, rows = _read(full / fname)
        assert head == ["frame"] + list(names) and len(rows) == T
        got = np.array([[float(v) for v in r[1:]] for r in rows]).T
        assert kc.worst(got, every[[kr.SERIES.index(n) for n in names]]) <= TOL
    n = int(want["n_turns"][0])
    head, rows = _read(turn / "turn_summary.csv")
    assert head == ["turn_id", "start_frame", "end_frame", "num_frames", "heading_change_deg", "direction"] and len(rows) == n
    for t, r in enumerate(rows):
        s, e = want["turn_frames"][0, t]
        assert [int(v) for v in r[:4]] == [t + 1, s, e, e - s + 1] and r[5] == ("left" if want["turn_direction"][0, t] > 0 else "right")
        assert abs(float(r[4]) - want["turn_heading_change"][0, t]) <= TOL * (1 + abs(float(r[4])))
    head, rows = _read(turn / "turn_metrics.csv")
    assert head == ["turn_id", "metric", "mean", "std", "min", "max"] and len(rows) == n * 42
    assert [r[1] for r in rows[:42]] == list(kr.SERIES) or n == 0
    got = np.array([[float(v) for v in r[2:]] for r in rows]).reshape(n, 42, 4)
    assert kc.worst(got, want["turn_stats"][0, :n]) <= TOL
    head, rows = _read(turn / "turn_heading.csv")
    assert head == ["frame", "heading_deg", "turn_boundary"] and len(rows) == T
    assert [int(r[2]) for r in rows] == want["boundary"][0].astype(int).tolist()
    assert kc.worst(np.array([float(r[1]) for r in rows]), want["heading"][0]) <= TOL
    for t in range(n):
        s, e = want["turn_frames"][0, t]
        d = turn / "turn_details" / f"turn_{t + 1}_{s}_{e}"
        head, rows = _read(d / "series.csv")
        assert head == ["local_frame", "global_frame", "heading_deg"] + list(kr.SERIES) and len(rows) == e - s + 1
        assert [int(r[1]) for r in rows] == list(range(s, e + 1))
        head, rows = _read(d / "summary.csv")
        assert head == ["turn_id", "start_frame", "end_frame", "num_frames", "metric", "mean", "std", "min", "max"] and len(rows) == 42
        for fname in angle.SERIES_FILES:
            assert (d / fname).exists()
    assert not list(out.rglob("*.png"))


def test_process_person(tmp_path):
    X = kc.CASES["g243"]["X"]
    np.save(tmp_path / "skier_fused.npy", X)
    angle.process_person(tmp_path / "skier_fused.npy", tmp_path / "out")
    _check_person(tmp_path / "out", kc.restated("g243"), 243)


def test_process_person_pair(tmp_path):
    np.save(tmp_path / "a_smoothed.npy", kc.CASES["g64"]["X"])
    np.save(tmp_path / "a_fused.npy", kc.CASES["t65"]["X"])
    angle.process_person_pair(tmp_path / "a_smoothed.npy", tmp_path / "a_fused.npy", tmp_path / "pair")
    before, after = kc.restated("g64"), kc.restated("t65")
    for sub, want, T in (("before_smoothed", before, 64), ("after_fused", after, 65)):
        head, rows = _read(tmp_path / "pair" / sub / "non_turn_evaluation" / "angles_change_fullframe.csv")
        assert head == ["frame"] + list(kr.SERIES[14:]) and len(rows) == T
        assert kc.worst(np.array([[float(v) for v in r[1:]] for r in rows]).T, want["changes"][0]) <= TOL
        assert (tmp_path / "pair" / sub / "turn_evaluation" / "turn_metrics.csv").exists()
    head, rows = _read(tmp_path / "pair" / "turn_compare_fused_vs_smoothed.csv")
    assert head == ["turn_pair_index", "before_turn_id", "after_turn_id", "metric", "before_mean", "after_mean", "delta_after_minus_before"]
    pairs = min(int(before["n_turns"][0]), int(after["n_turns"][0]))
    assert pairs == 3 and len(rows) == pairs * 42
    metrics = sorted(kr.SERIES)
    assert [r[3] for r in rows[:42]] == metrics
    order = [kr.SERIES.index(m) for m in metrics]
    got = np.array([[float(v) for v in r[4:]] for r in rows]).reshape(pairs, 42, 3)
    mb, ma = before["turn_stats"][0, :pairs, order, 0].T, after["turn_stats"][0, :pairs, order, 0].T
    assert kc.worst(got[..., 0], mb) <= TOL and kc.worst(got[..., 1], ma) <= TOL and kc.worst(got[..., 2], ma - mb) <= 2 * TOL
    assert [[int(v) for v in r[:3]] for r in rows[::42]] == [[i + 1, i + 1, i + 1] for i in range(pairs)]


def test_process_video_3d_analyze(tmp_path):
    fw = [3, 3, 3]
    sd = W.make_vp3d_state_dict(seed=0, filter_widths=fw)
    torch.save({"epoch": 80, "model_pos": sd}, tmp_path / "ckpt.bin")
    for name, T, seed in (("osmo_1", 21, 2), ("osmo_2", 24, 5)):
        torch.save({"video_name": name, "video_path": "", "img_shape": (1080, 1920),
                    "detectron2": {"keypoints": W.make_keypoints_2d(frames=T, seed=seed)}, "depth": None}, tmp_path / f"{name}.pt")
    args = SimpleNamespace(architecture="3,3,3", causal=False, dropout=0.25, channels=1024, dense=False, test_time_augmentation=True)
    config = {"model": {"ckpt_path": str(tmp_path / "ckpt.bin")}}
    files = {}
    for tag, kw in (("off", {}), ("on", dict(analyze=True))):
        fused, _ = run.process_video_3d(config, tmp_path / "osmo_1.pt", tmp_path / "osmo_2.pt", tmp_path / tag, tmp_path / tag / "npy" / "skier",
                                        args, **kw)
        files[tag] = (tmp_path / tag / "npy" / "skier_fused_keypoints.npy").read_bytes()
    assert files["on"] == files["off"]
    assert not (tmp_path / "off" / "angle").exists()
    # the lifter's weights are random, so its poses are too: only the per-frame series, which hang on no decision over time,
    # are compared here; the turn files are checked for being there (their content: test_process_person)
    want = kr.kinematics(fused.cpu().numpy(), layout=kr.H36M_17)
    out = tmp_path / "on" / "angle"
    head, rows = _read(out / "non_turn_evaluation" / "angles_joint.csv")
    assert head == ["frame"] + list(kr.SERIES[:8]) and len(rows) == 21
    assert kc.worst(np.array([[float(v) for v in r[1:]] for r in rows]).T, want["series"][0, :8]) <= TOL
    for fname in angle.SERIES_FILES:
        assert (out / "non_turn_evaluation" / fname).exists()
    for fname in ("turn_summary.csv", "turn_metrics.csv", "turn_heading.csv"):
        assert (out / "turn_evaluation" / fname).exists()
    assert (out / "turn_evaluation" / "turn_details").is_dir() and not list(out.rglob("*.png"))
