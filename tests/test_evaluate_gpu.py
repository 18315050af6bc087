"""GPU: the pose evaluation of clips (csrc/evaluate.hip: skimi_pose_errors, skimi_clip_quality) against the float64
restatement (tests/evaluate_restated.py, itself held against the reference's outputs by tests/test_evaluate_cpu.py) on
every case of tests/evaluate_cases.py: NaN masks, counts and p_status equal, every float within 1e-9 (1 + |x|), the
project's float64 tolerance.  Results must be bitwise reproducible, a clip's the same alone and inside the ragged batch
with garbage in the padding, a [T, J, 3] input the same as [1, T, J, 3], and the same in both placements of the per-clip
arrays.  Then evaluate.py on top (eval_fused_pose against the reference's dict, evaluate_clips against the rerun of the
reference's loop, the four protocols, the per-joint summary, the smoothing gain) and run.process_video_3d(evaluate=True)."""
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import evaluate_cases as ec
import evaluate_restated as er
from skiing_analysis_pytorch_amd import _lib, evaluate, geometry, run, weights as W

pytestmark = pytest.mark.gpu
TOL = 1e-9
GOLD = np.load(Path(__file__).resolve().parent / "golden" / "evaluate.npz")
PE_FLOATS = er.PE_FRAME_FLOATS + er.PE_CLIP_FLOATS


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def device_pe(case, **over):
    r = geometry.pose_errors(dev(case["pred"]), dev(case["target"]), aligned=True, **{**ec.params(case), **over})
    torch.cuda.synchronize()
    return r


def device_cq(case, X=None, **over):
    X = case["pred"] if X is None else X
    r = geometry.clip_quality(dev(X), **{"lengths": case.get("lengths"), **ec.layout(X.shape[-2]), **over})
    torch.cuda.synchronize()
    return r


def bits(x):
    return np.ascontiguousarray(x.cpu().numpy()).tobytes()


def same_bits(a, b):
    return all(getattr(a, k).shape == getattr(b, k).shape and bits(getattr(a, k)) == bits(getattr(b, k)) for k in a._fields)


def check(name, r, want, floats, exact):
    for k in exact:
        got = getattr(r, k).cpu().numpy()
        assert got.shape == want[k].shape and np.array_equal(got, want[k]), f"{name}: {k} differs"
    w = {k: er.worst(getattr(r, k).cpu().numpy(), want[k]) for k in floats}
    print(f"{name}: worst |dev - restatement| / (1 + |x|): " + ", ".join(f"{k} {v:.1e}" for k, v in w.items()))
    for k, v in w.items():
        assert v <= TOL, f"{name}: {k} off by {v:.3e} (inf: the shapes or NaN masks differ)"


@pytest.mark.parametrize("name", list(ec.CASES))
def test_against_restatement(name):
    case = ec.CASES[name]
    pe, cq = ec.restated(name)
    r = device_pe(case)
    assert r.p_status.dtype == torch.bool and r.n_valid_f.dtype == torch.int32 and r.n_err.dtype == torch.int32
    check(name, r, pe, PE_FLOATS, er.PE_EXACT)
    q = device_cq(case)
    check(name, q, cq, er.CQ_FLOATS, ())


@pytest.mark.parametrize("name", ["missing_T21_J17", "clean_T300_J17", "ragged_B3_T41_J17", "clean_T21_J70"])
def test_reruns_are_bitwise_equal(name):
    case = ec.CASES[name]
    assert same_bits(device_pe(case), device_pe(case))
    assert same_bits(device_cq(case), device_cq(case))


def test_clip_alone_and_in_the_ragged_batch():
    case = ec.CASES["ragged_B3_T41_J17"]
    rb, qb = device_pe(case), device_cq(case)
    for b, n in enumerate(case["lengths"]):
        alone = dict(pred=case["pred"][b, :n], target=case["target"][b, :n])
        ra, qa = device_pe(alone), device_cq(alone)
        for res_a, res_b, frame_fields in ((ra, rb, er.PE_FRAME_FLOATS + ("n_valid_f", "p_status")), (qa, qb, ("bone_len",))):
            for k in res_a._fields:
                x, y = getattr(res_a, k)[0], getattr(res_b, k)[b]
                if k in frame_fields:
                    y = y[:n]
                assert x.shape == y.shape and bits(x) == bits(y), f"clip {b} (length {n}): {k} differs between alone and in the batch"


@pytest.mark.parametrize("name", ["gaps_T41_J15", "clean_T4_J70"])
def test_one_clip_with_and_without_the_batch_axis(name):
    case = ec.CASES[name]
    assert same_bits(device_pe(case), device_pe(dict(pred=case["pred"][None], target=case["target"][None])))
    assert same_bits(device_cq(case), device_cq(case, X=case["pred"][None]))


@pytest.mark.parametrize("name", ["clean_T3_J17", "clean_T21_J17", "gaps_T41_J15", "missing_T21_J17", "clean_T4_J70", "clean_T21_J1",
                                  "ragged_B3_T41_J17"])
def test_lds_and_workspace_placement_agree(name):
    case = ec.CASES[name]
    T, J = case["pred"].shape[-3:-1]
    assert T * J <= geometry.EVAL_LDS_ELEMS                 # "auto" is the LDS here
    assert same_bits(device_cq(case), device_cq(case, placement="workspace"))


def test_placement_threshold():
    assert 300 * 17 > geometry.EVAL_LDS_ELEMS               # clean_T300_J17 ran from the workspace in test_against_restatement
    X = dev(ec.CASES["clean_T300_J17"]["pred"])
    lib = _lib.lib()
    sc = torch.empty(8, dtype=torch.float64, device="cuda")
    import ctypes as C
    none = (C.c_int32 * 1)()
    rc = lib.skimi_clip_quality(X.data_ptr(), None, 1, 300, 17, none, 0, none, 0, none, 0, none, 0, None, 0, sc.data_ptr(), None, None, None)
    assert rc == -1 and b"needs a workspace" in lib.skimi_last_error()
    ws = torch.empty(8, dtype=torch.float64, device="cuda")
    rc = lib.skimi_clip_quality(X.data_ptr(), None, 1, 300, 17, none, 0, none, 0, none, 0, none, 0, ws.data_ptr(), 64, sc.data_ptr(), None,
                                None, None)
    assert rc == -1 and b"skimi_eval_workspace_bytes asks for" in lib.skimi_last_error()
    with pytest.raises(ValueError):
        geometry.clip_quality(X, placement="lds")
    with pytest.raises(_lib.SkimiError):
        geometry.pose_errors(torch.zeros(2, 129, 3, device="cuda"), torch.zeros(2, 129, 3, device="cuda"))
    with pytest.raises(ValueError):
        geometry.pose_errors(X, X[:4])
    with pytest.raises(ValueError):
        geometry.pose_errors(X, X, lengths=[1, 2])


@pytest.mark.parametrize("name", ec.FUSED)
def test_eval_fused_pose(name):
    left, right, fused = ec.fused_inputs(name)
    m = evaluate.eval_fused_pose(dev(left), dev(right), dev(fused))
    keys, values = [str(k) for k in GOLD[f"fused_{name}_keys"]], GOLD[f"fused_{name}_values"]
    assert list(m) == keys and all(isinstance(v, float) for v in m.values())
    w = er.worst(np.array(list(m.values())), values)
    print(f"eval_fused_pose {name}: worst |dev - reference| / (1 + |x|) {w:.1e}")
    assert w <= TOL
    again = evaluate.eval_fused_pose(left, right, fused)               # host arrays are uploaded
    assert list(again) == keys and np.array_equal(np.array(list(again.values())), np.array(list(m.values())), equal_nan=True)


@pytest.mark.parametrize("group", list(ec.EVAL_CLIPS))
def test_evaluate_clips(group):
    names = ec.EVAL_CLIPS[group]
    got = evaluate.evaluate_clips([dev(ec.CASES[n]["pred"]) for n in names], [dev(ec.CASES[n]["target"]) for n in names], zero_root=0)
    assert len(got) == 4 and all(v.is_cuda and v.dim() == 0 and v.dtype == torch.float64 for v in got)
    w = er.worst(np.array([float(v) for v in got]), GOLD[f"loop_{group}"])
    print(f"evaluate_clips {group}: {[float(v) for v in got]} mm, worst |dev - reference loop| / (1 + |x|) {w:.1e}")
    assert w <= TOL


def test_protocol_functions():
    name = "clean_T21_J17"
    p, g = dev(ec.CASES[name]["pred"]), dev(ec.CASES[name]["target"])
    got = [evaluate.mpjpe(p, g), evaluate.p_mpjpe(p, g), evaluate.n_mpjpe(p[None], g[None]), evaluate.mean_velocity_error(p, g)]
    assert all(v.is_cuda and v.dim() == 0 for v in got)
    assert er.worst(np.array([float(v) for v in got]), GOLD[f"{name}_0_loss"]) <= TOL
    with pytest.raises(ValueError):
        evaluate.mpjpe(p, g[:4])


def test_joint_error_summary_and_smoothing_gain():
    case = ec.CASES["gaps_T41_J15"]
    ids = (1, 2, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 41, 62, 69)
    s = evaluate.joint_error_summary(dev(case["pred"]), dev(case["target"]), target_ids=ids)
    want = GOLD["gaps_T41_J15_0_joint_summary"]
    assert list(s) == list(ids)
    got = np.array([[s[j][k] for k in ("mean", "std", "median", "n")] for j in ids], dtype=np.float64)
    assert er.worst(got, want) <= TOL and all(isinstance(s[j]["n"], int) for j in ids)
    raw = case["pred"]
    smooth = er.fill_series(raw)
    smooth[1:-1] = (smooth[:-2] + smooth[1:-1] + smooth[2:]) / 3.0
    g = evaluate.smoothing_gain(dev(raw), dev(smooth))
    lay = ec.layout(15)
    qr, qs = (er.clip_quality_clip(x, lay["edges"], (), (), ()) for x in (raw, smooth))
    want = dict(raw_speed=qr["speed_mean"], smooth_speed=qs["speed_mean"], raw_jerk=qr["jerk_mean"], smooth_jerk=qs["jerk_mean"],
                raw_bone_cv=qr["bone_cv_mean"], smooth_bone_cv=qs["bone_cv_mean"])
    want.update(jerk_gain_pct=(want["raw_jerk"] - want["smooth_jerk"]) / want["raw_jerk"] * 100,
                speed_gain_pct=(want["raw_speed"] - want["smooth_speed"]) / want["raw_speed"] * 100,
                bone_cv_gain_pct=(want["raw_bone_cv"] - want["smooth_bone_cv"]) / want["raw_bone_cv"] * 100)
    assert list(g) == list(want)
    gv, wv = np.array(list(g.values())), np.array(list(want.values()))
    assert er.worst(gv[:6], wv[:6]) <= TOL
    # a percentage is 100 (a - b) / a: figures within 1e-9 of theirs move it by at most 100 * 2e-9 * (a + b) / a < 1e-6
    assert np.abs(gv[6:] - wv[6:]).max() <= 1e-6
    assert g["jerk_gain_pct"] > 0


def test_process_video_3d_evaluate(tmp_path):
    fw = [3, 3, 3]
    sd = W.make_vp3d_state_dict(seed=0, filter_widths=fw)
    torch.save({"epoch": 80, "model_pos": sd}, tmp_path / "ckpt.bin")
    for name, T, seed in (("osmo_1", 21, 2), ("osmo_2", 24, 5)):
        torch.save({"video_name": name, "video_path": "", "img_shape": (1080, 1920),
                    "detectron2": {"keypoints": W.make_keypoints_2d(frames=T, seed=seed)}, "depth": None}, tmp_path / f"{name}.pt")
    args = SimpleNamespace(architecture="3,3,3", causal=False, dropout=0.25, channels=1024, dense=False, test_time_augmentation=True)
    config = {"model": {"ckpt_path": str(tmp_path / "ckpt.bin")}}
    files = {}
    for tag, kw in (("plain", {}), ("off", dict(evaluate=False)), ("on", dict(evaluate=True))):
        fused, _ = run.process_video_3d(config, tmp_path / "osmo_1.pt", tmp_path / "osmo_2.pt", tmp_path / tag, tmp_path / tag / "npy" / "skier",
                                        args, **kw)
        files[tag] = {str(p.relative_to(tmp_path / tag)): p.read_bytes() for p in sorted((tmp_path / tag).rglob("*")) if p.is_file()}
    assert files["plain"] == files["off"]                       # the call without the flag and with it off: the same files, byte for byte
    assert set(files["on"]) == set(files["off"]) | {"fused_metrics.txt"}
    assert all(files["on"][k] == v for k, v in files["off"].items())
    left = np.load(tmp_path / "on" / "videopose3d" / "left" / "osmo_1.npy")
    saved = np.load(tmp_path / "on" / "npy" / "skier_fused_keypoints.npy", allow_pickle=True)
    text = files["on"]["fused_metrics.txt"].decode("utf-8")
    lines = text.splitlines()
    assert lines[0] == "Fused Pose Evaluation Metrics:" and len(lines) == 10 and text.endswith("\n")
    assert [ln[:25].rstrip() for ln in lines[1:]] == list(evaluate.FUSED_METRIC_KEYS) and all(ln[25:27] == ": " for ln in lines[1:])
    # the values: the restatement on what the run fused (the views as the run passes them: lifted, turned, cut to 21 frames)
    assert left.shape[0] == 21 and saved is not None
    lw, _ = run.run_video_pose_3d(config, tmp_path / "osmo_1.pt", tmp_path / "again" / "l", args)
    rw, _ = run.run_video_pose_3d(config, tmp_path / "osmo_2.pt", tmp_path / "again" / "r", args)
    want = er.eval_fused_pose(lw[:21].astype(np.float64), rw[:21].astype(np.float64), fused.cpu().numpy())
    assert text == evaluate.format_fused_metrics(want)
