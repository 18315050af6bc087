"""CPU: the restatement of the kinematic analysis (tests/kinematics_restated.py) against the reference's own outputs
(tests/golden/kinematics.npz, written by tools/make_goldens.py kinematics from angle/main.py), the stability of every case
of tests/kinematics_cases.py, and the CSV writers of skiing_analysis_pytorch_amd/angle.py driven from restated arrays.

Stability.  The device is compared with the restatement to 1e-9, which says nothing where a result hangs on a comparison:
the tilt's sign (p.f >= 0), the unwrap's jumps (|dd| < pi), the velocity's sign changes, the boundaries picked from them and
the turn filter (|change| >= threshold; the length test is on integers).  Each of these must have a margin in every case:
|p.f| >= 1e-6, ||dd| - pi| >= 1e-6 rad, |v| >= 1e-6 deg/frame on both sides of a sign change, ||change| - threshold| >= 1e-6
deg; and a relative perturbation of X by 1e-12 must change no discrete output.  One case sits on a decision on purpose:
"constant_heading" has every velocity exactly 0 (0 * 0 is no sign change), which holds only for the exact input, so its
extrema are not compared under the perturbation -- its outputs are: no segment comes within 7.99 degrees of the filter.
Likewise "zero_limb" is two joints in one place, which the perturbation keeps together."""
import csv
import importlib.util
import os
from pathlib import Path

import numpy as np
import pytest

import kinematics_cases as kc
import kinematics_restated as kr
from skiing_analysis_pytorch_amd import angle, geometry

GOLD = np.load(Path(__file__).resolve().parent / "golden" / "kinematics.npz")
TOL = 1e-12
ALL_CASES = list(kc.CASES) + ["straight"]


def case_of(name):
    return kc.straight_case() if name == "straight" else kc.CASES[name]


def test_tables():
    assert list(GOLD["names"]) == list(kr.SERIES) == list(geometry.KIN_SERIES) == list(angle.SERIES) and len(kr.SERIES) == 42
    assert kr.ROLES == geometry.KIN_ROLES and kr.BASE == geometry.KIN_BASE_SERIES
    assert kr.MHR70_15 == angle.MHR70_15 == geometry.KIN_LAYOUT_MHR70_15 and kr.H36M_17 == angle.H36M_17
    # the layout is the reference's ids as positions in its 15-joint order, the angles its triples
    assert [angle.TARGET_IDS[j] for j in angle.MHR70_15] == [5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 62, 41, 69]
    for name, ids in angle.ANGLE_DEFS.items():
        assert tuple(angle.ROLE_IDS[kr.ROLES.index(r)] for r in kr.ANGLES[name]) == ids
    assert [name for names in list(angle.SERIES_FILES.values())[2:] for name in names] == list(kr.SERIES[8:])
    for T in (0, 1, 11, 12, 13, 24, 25, 243, 4099):
        for m in (1, 5, 12):
            assert kr.max_turns(T, m) == geometry.kin_max_turns(T, m)
    assert sorted(GOLD["clips"]) == sorted(kc.GOLDEN) and {kc.GOLDEN[c]["X"].shape[0] for c in kc.GOLDEN} == {11, 13, 64, 243}


@pytest.mark.parametrize("name", list(kc.GOLDEN))
def test_restatement_against_reference(name):
    case, r = kc.GOLDEN[name], kc.restated(name)
    assert np.array_equal(case["X"], GOLD[f"{name}_X"], equal_nan=True)
    assert np.array_equal(np.asarray(case.get("up_axis", (0.0, -1.0, 0.0))), GOLD[f"{name}_up"])
    w = {"series": kc.worst(np.concatenate([r["series"][0], r["changes"][0]]), GOLD[f"{name}_series"]),
         "heading": kc.worst(r["heading"][0], GOLD[f"{name}_heading"])}
    turns, n = GOLD[f"{name}_turns"], int(r["n_turns"][0])
    assert n == len(turns) and np.array_equal(r["boundary"][0], GOLD[f"{name}_boundary"].astype(bool))
    assert np.array_equal(r["turn_frames"][0, :n], turns[:, 1:3].astype(np.int32))
    assert np.array_equal(turns[:, 0], np.arange(1, n + 1)) and np.array_equal(turns[:, 3], turns[:, 2] - turns[:, 1] + 1)
    assert np.array_equal(r["turn_direction"][0, :n], turns[:, 5].astype(np.int32))
    w["turn_heading_change"] = kc.worst(r["turn_heading_change"][0, :n], turns[:, 4])
    w["turn_stats"] = kc.worst(r["turn_stats"][0, :n], GOLD[f"{name}_stats"])
    assert np.array_equal(r["turn_counts"][0, :n] == 0, np.isnan(GOLD[f"{name}_stats"][..., 0]))
    print(f"{name}: worst |restatement - reference| / (1 + |x|): " + ", ".join(f"{k} {v:.1e}" for k, v in w.items()))
    assert max(w.values()) <= TOL


def test_goldens_cover_what_they_must():
    turns = {c: len(GOLD[f"{c}_turns"]) for c in kc.GOLDEN}
    assert turns["g64"] == 3 and turns["g243"] == 9 and turns["g11"] == 0
    h = GOLD["g243_heading"]
    with np.errstate(invalid="ignore"):
        assert (np.abs(np.diff(h)) > 180.0).sum() >= 8 and np.nanmax(h) > 170.0 and np.nanmin(h) < -170.0    # the heading crosses +-180
    assert np.isnan(h[:2]).all() and np.isnan(h[100:105]).all() and np.isnan(h[241:]).all() and np.isfinite(h[150:170]).all()
    assert np.isnan(GOLD["g13_heading"][[0, 12]]).all() and np.isfinite(GOLD["g64_heading"][20:30]).all()
    assert np.isnan(GOLD["g64_X"][20:30, kr.MHR70_15[4]]).all() and GOLD["g64_up_up"][1] == 1.0


@pytest.mark.parametrize("name", ALL_CASES)
def test_margins(name):
    case, r = case_of(name), kc.restated(name)
    thr, m = case.get("min_heading_change_deg", 8.0), case.get("min_turn_frames", 12)
    worst = dict(v=np.inf, dd=np.inf, dh=np.inf, dot=np.inf, cos=0.0)
    for d in r["debug"]:
        vs, ex = d["velocity_smooth"], d["extrema"]
        if ex.size:
            worst["v"] = min(worst["v"], float(np.minimum(np.abs(vs[ex - 1]), np.abs(vs[ex])).min()))
        if d["dd"].size:
            worst["dd"] = min(worst["dd"], float(np.abs(np.abs(d["dd"]) - np.pi).min()))
        for s, e, dh in d["segments"]:
            if e - s + 1 >= m:
                worst["dh"] = min(worst["dh"], abs(abs(dh) - thr))
        dots = d["tilt_dots"][np.isfinite(d["tilt_dots"])]
        if dots.size:
            worst["dot"] = min(worst["dot"], float(np.abs(dots).min()))
        cos = d["cosines"][np.isfinite(d["cosines"])]
        if cos.size:
            worst["cos"] = max(worst["cos"], float(np.abs(cos).max()))
    print(f"{name}: smallest margins: |v| at a sign change {worst['v']:.2e}, ||dd| - pi| {worst['dd']:.2e}, ||dh| - thr| {worst['dh']:.2e}, "
          f"|p.f| {worst['dot']:.2e}; largest |cos| {worst['cos']:.4f}")
    assert worst["v"] >= 1e-6 and worst["dd"] >= 1e-6 and worst["dh"] >= 1e-6 and worst["dot"] >= 1e-6
    if name == "straight":
        assert worst["cos"] > 1.0 - 1e-12
    else:
        assert worst["cos"] < 0.999
    if name == "constant_heading":
        d = r["debug"][0]
        assert not d["velocity_smooth"].any() and d["extrema"].size == 0 and not r["heading"].any() and r["n_turns"][0] == 0


@pytest.mark.parametrize("name", ALL_CASES)
def test_perturbation_changes_no_decision(name):
    case, r = case_of(name), kc.restated(name)
    X = case["X"]
    u = np.random.default_rng(5).uniform(-1.0, 1.0, size=X.shape)
    with np.errstate(invalid="ignore", over="ignore"):
        Xp = X * (1.0 + 1e-12 * u)
        if name == "zero_limb":
            Xp = kc.zero_limb_ties(Xp)      # the case is two joints in one place: the perturbation moves them together
        p = kr.kinematics(Xp, **kc.params(case))
    for k in kc.EXACT_FIELDS:
        assert np.array_equal(r[k], p[k]), k
    for k in kc.FLOAT_FIELDS:
        assert np.array_equal(np.isnan(r[k]), np.isnan(p[k])), k
    tilt = slice(12, 14)
    assert np.array_equal(np.sign(r["series"][:, tilt]), np.sign(p["series"][:, tilt]), equal_nan=True)
    for a, b in zip(r["debug"], p["debug"]):
        assert [s[:2] for s in a["kept"]] == [s[:2] for s in b["kept"]]
        assert np.array_equal(np.abs(a["dd"]) < np.pi, np.abs(b["dd"]) < np.pi)
        if name != "constant_heading":
            assert np.array_equal(a["extrema"], b["extrema"]) and [s[:2] for s in a["segments"]] == [s[:2] for s in b["segments"]]
        else:
            assert all(abs(s[2]) < 1e-2 for s in b["segments"])


def test_cases_cover_what_they_must():
    n = {k: kc.restated(k)["n_turns"] for k in kc.CASES}
    assert all(n[f"t{T}"][0] == 0 for T in (0, 1, 4, 5, 10, 11)) and n["t12"][0] == 1 and n["t13"][0] == 1
    assert n["t4099"][0] > 100 and kc.CASES["t4099"]["X"].shape[0] > geometry.KIN_LDS_FRAMES
    assert not np.isfinite(kc.restated("no_heading")["heading"]).any() and np.isfinite(kc.restated("one_heading")["heading"]).sum() == 1
    # a short last segment: the last boundary pair is closer than min_turn_frames and is dropped
    d = kc.restated("short_last")["debug"][0]
    s, e, _ = d["segments"][-1]
    assert e == 53 and e - s + 1 < 12 and len(d["kept"]) == len(d["segments"]) - 1
    # turns rejected by the heading change alone
    d = kc.restated("small_change")["debug"][0]
    assert any(e - s + 1 >= 12 and abs(dh) < 8.0 for s, e, dh in d["segments"]) and len(d["kept"]) >= 2
    z = kc.restated("zero_limb")["series"][0]
    assert np.isnan(z[0, 5:9]).all() and np.isfinite(z[0, 4]) and np.isnan(z[6, 12:14]).all()
    a = kc.restated("absent_role")["series"][0]
    assert np.isnan(a[[2, 4, 5, 6, 7]]).all() and np.isfinite(a[[0, 1, 3, 8]]).all()
    assert list(kc.restated("ragged")["n_turns"]) == [3, 3, 1]
    # clips shorter than a window follow the in-range rule: finite everywhere
    for T in (5, 10):
        r = kc.restated(f"t{T}")
        assert np.isfinite(r["heading_smooth"]).all() and np.isfinite(r["velocity_smooth"]).all()
    r = kc.restated("t5")
    h = np.degrees(np.unwrap(np.radians(r["heading"][0])))
    assert np.abs(r["heading_smooth"][0] - h.mean()).max() < 1e-12 * 200        # window 11 over 5 samples: all of them, everywhere


def test_reference_raises_on_short_clips_and_the_restatement_does_not(monkeypatch):
    r = kc.restated("t10")
    assert r["n_turns"][0] == 0 and np.isfinite(r["heading_smooth"]).all()
    ref = Path(os.environ.get("SKIMI_REFERENCE", "/root/reference")) / "angle" / "main.py"
    if not ref.exists():
        return                                                          # the rest needs the reference's tree
    monkeypatch.setenv("MPLBACKEND", "Agg")
    spec = importlib.util.spec_from_file_location("ref_angle_main", ref)
    A = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(A)
    with pytest.raises(IndexError):
        A.detect_turn_segments(r["heading"][0])
    assert len(A.detect_turn_segments(kc.restated("t11")["heading"][0])) == 0


# ---- the CSV writers, driven from restated arrays ----------------------------------------------------------------------
def _read(path):
    with open(path, newline="") as f:
        rows = list(csv.reader(f))
    return rows[0], rows[1:]


def _floats(rows, start):
    return np.array([[float(v) for v in r[start:]] for r in rows], dtype=np.float64)


def test_write_person(tmp_path):
    r = kc.restated("g243")
    a = angle.analysis_from(r)
    angle.write_person(a, tmp_path)
    every = np.concatenate([r["series"][0], r["changes"][0]])
    full, turn = tmp_path / "non_turn_evaluation", tmp_path / "turn_evaluation"
    assert sorted(p.name for p in full.iterdir()) == sorted(angle.SERIES_FILES)
    for fname, names in angle.SERIES_FILES.items():
        head, rows = _read(full / fname)
        assert head == ["frame"] + list(names) and [int(x[0]) for x in rows] == list(range(243))
        assert np.array_equal(_floats(rows, 1).T, every[[kr.SERIES.index(n) for n in names]], equal_nan=True)   # repr round-trips
    n = int(r["n_turns"][0])
    assert n == 9
    head, rows = _read(turn / "turn_summary.csv")
    assert head == list(angle.TURN_FIELDS) and len(rows) == n
    for t, row in enumerate(rows):
        s, e = (int(v) for v in r["turn_frames"][0, t])
        assert row[:4] == [str(t + 1), str(s), str(e), str(e - s + 1)] and float(row[4]) == r["turn_heading_change"][0, t]
        assert row[5] == ("left" if r["turn_direction"][0, t] > 0 else "right")
    head, rows = _read(turn / "turn_metrics.csv")
    assert head == ["turn_id", "metric", "mean", "std", "min", "max"] and len(rows) == n * 42
    assert [x[1] for x in rows[:42]] == list(kr.SERIES) and [x[0] for x in rows[::42]] == [str(t + 1) for t in range(n)]
    assert np.array_equal(_floats(rows, 2).reshape(n, 42, 4), r["turn_stats"][0, :n], equal_nan=True)
    assert any(x[2:] == ["nan"] * 4 for x in rows)                      # a series with no finite sample in a turn
    head, rows = _read(turn / "turn_heading.csv")
    assert head == ["frame", "heading_deg", "turn_boundary"] and len(rows) == 243
    assert [int(x[2]) for x in rows] == r["boundary"][0].astype(int).tolist()
    assert np.array_equal(_floats(rows, 1)[:, 0], r["heading"][0], equal_nan=True)
    dirs = sorted(p.name for p in (turn / "turn_details").iterdir())
    assert dirs == sorted(f"turn_{t + 1}_{r['turn_frames'][0, t, 0]}_{r['turn_frames'][0, t, 1]}" for t in range(n))
    s, e = (int(v) for v in r["turn_frames"][0, 1])
    d = turn / "turn_details" / f"turn_2_{s}_{e}"
    assert sorted(p.name for p in d.iterdir()) == sorted(list(angle.SERIES_FILES) + ["series.csv", "summary.csv"])
    head, rows = _read(d / "series.csv")
    assert head == ["local_frame", "global_frame", "heading_deg"] + list(kr.SERIES)
    assert [(int(x[0]), int(x[1])) for x in rows] == [(g - s, g) for g in range(s, e + 1)]
    assert np.array_equal(_floats(rows, 3).T, every[:, s:e + 1], equal_nan=True)
    head, rows = _read(d / "summary.csv")
    assert head == ["turn_id", "start_frame", "end_frame", "num_frames", "metric", "mean", "std", "min", "max"]
    assert all(x[:4] == ["2", str(s), str(e), str(e - s + 1)] for x in rows) and [x[4] for x in rows] == list(kr.SERIES)
    assert np.array_equal(_floats(rows, 5), r["turn_stats"][0, 1], equal_nan=True)
    head, rows = _read(d / "angles_knee.csv")
    assert head == ["frame", "knee_l", "knee_r"] and [int(x[0]) for x in rows] == list(range(e - s + 1))
    assert np.array_equal(_floats(rows, 1).T, every[:2, s:e + 1], equal_nan=True)
    assert not list(tmp_path.rglob("*.png"))


def test_write_person_pair(tmp_path):
    rb, ra = kc.restated("g64"), kc.restated("t1025")
    before, after = angle.analysis_from(rb), angle.analysis_from(ra)
    angle.write_person_pair(before, after, tmp_path)
    for sub in ("before_smoothed", "after_fused"):
        assert [p.name for p in (tmp_path / sub / "non_turn_evaluation").iterdir()] == ["angles_change_fullframe.csv"]
        assert (tmp_path / sub / "turn_evaluation" / "turn_summary.csv").exists()
    head, rows = _read(tmp_path / "turn_compare_fused_vs_smoothed.csv")
    assert head == ["turn_pair_index", "before_turn_id", "after_turn_id", "metric", "before_mean", "after_mean", "delta_after_minus_before"]
    assert len(rows) == 3 * 42 and [x[3] for x in rows[:42]] == sorted(kr.SERIES)
    order = [kr.SERIES.index(m) for m in sorted(kr.SERIES)]
    got = _floats(rows, 4).reshape(3, 42, 3)
    mb, ma = rb["turn_stats"][0, :3][:, order, 0], ra["turn_stats"][0, :3][:, order, 0]
    assert np.array_equal(got[..., 0], mb, equal_nan=True) and np.array_equal(got[..., 1], ma, equal_nan=True)
    assert np.array_equal(got[..., 2], ma - mb, equal_nan=True)


def test_compute_all_series_shape_of_the_tuple(monkeypatch):
    monkeypatch.setattr(angle, "analyze", lambda kpts, up, layout: angle.analysis_from(kr.kinematics(kpts, layout=layout, up_axis=up)))
    out = angle.compute_all_series(kc.GOLDEN["g64"]["X"])
    assert [list(d) for d in out[:5]] == [list(kr.SERIES[:8]), ["tilt_upper", "tilt_lower"], ["torso_knee_angle"], ["knee_diff_lr"],
                                          ["elbow_distance_l", "elbow_distance_r"]]
    assert out[5].shape == (64,) and [set(t) for t in out[6]] == [set(angle.TURN_FIELDS)] * 3
    assert [t["turn_id"] for t in out[6]] == [1.0, 2.0, 3.0] and all(isinstance(v, float) for t in out[6] for v in t.values())
