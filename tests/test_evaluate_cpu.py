"""CPU: the restatement of the pose evaluation (tests/evaluate_restated.py) against the reference's own functions
(tests/golden/evaluate.npz: VideoPose3D/common/loss.py, VideoPose3D/fuse/fuse_eval.py, metrics/unity_data_compare.py and
metrics/true_data_compare.py run by tools/make_goldens.py on the clips of tests/evaluate_cases.py) within 1e-12 (1 + |x|)
with equal NaN masks and counts; the rules stated where the reference raises or leaves a key out; evaluate_clips' weighting
against a float64 rerun of the loop of VideoPose3D/run.py:998-1041; the text of fused_metrics.txt; argument validation, which
the library does before any launch and so without a GPU."""
import ctypes as C
import hashlib
from pathlib import Path

import numpy as np
import pytest
import torch

import evaluate_cases as ec
import evaluate_restated as er
from skiing_analysis_pytorch_amd import _lib, evaluate, geometry

GOLD = np.load(Path(__file__).resolve().parent / "golden" / "evaluate.npz")
TOL = 1e-12


def close(got, want, what, tol=TOL):
    w = er.worst(np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64))
    assert w <= tol, f"{what}: off by {w:.3e} (inf: the shapes or NaN masks differ)"
    return w


def test_golden_is_of_these_cases():
    assert list(GOLD["cases"]) == list(ec.CASES)
    for name, c in ec.CASES.items():
        for k in ("pred", "target"):
            g = GOLD[f"{name}_{k}"]
            if g.dtype.kind == "U":
                assert hashlib.sha256(np.ascontiguousarray(c[k]).tobytes()).hexdigest() == str(g), f"{name}: {k}"
            else:
                assert g.shape == c[k].shape and np.array_equal(g, c[k], equal_nan=True), f"{name}: {k}"


def test_singular_values_are_apart():
    print("smallest gap of H's two smallest singular values: " + ", ".join(f"{k} {v:.3f}" for k, v in ec.SV_GAPS.items() if np.isfinite(v)))
    assert min(ec.SV_GAPS.values()) >= ec.MIN_SV_GAP


@pytest.mark.parametrize("name", list(ec.CASES))
def test_restatement_against_reference(name):
    case = ec.CASES[name]
    pe, cq = ec.restated(name)
    J = case["pred"].shape[-2]
    for b, (p, _) in enumerate(ec.clips_of(case)):
        n, key = p.shape[0], f"{name}_{b}"
        if n >= 1:
            close(pe["mpjpe"][b], GOLD[f"{key}_mpd"], "mean_pairwise_distance")
            summ = GOLD[f"{key}_joint_summary"]
            close(pe["joint_err"][b], summ[:, :3], "summarize_joint_errors")
            assert np.array_equal(pe["joint_err_n"][b], summ[:, 3].astype(np.int32))
            if f"{key}_per_joint_err" in GOLD:
                close(pe["err"][b, :n], GOLD[f"{key}_per_joint_err"], "calculate_per_joint_errors")
        if f"{key}_loss" in GOLD:
            e1, e2, e3, ev = GOLD[f"{key}_loss"]
            close(pe["mpjpe"][b], e1, "mpjpe")
            close(pe["p_mpjpe"][b], e2, "p_mpjpe")
            close(pe["n_mpjpe"][b], e3, "n_mpjpe")
            close(pe["mpjve"][b], ev, "mean_velocity_error")
            assert pe["n_complete"][b] == n and pe["p_status"][b, :n].all() and pe["n_err"][b] == n * J
            assert pe["n_vel"][b] == max(n - 1, 0) * J
        if f"{key}_bone_len" in GOLD:
            close(cq["bone_len"][b, :n], GOLD[f"{key}_bone_len"], "bone_lengths")
        close([cq["speed_p95"][b], cq["accel_p95"][b]], GOLD[f"{key}_p95"], "temporal_stats")
        if f"{key}_mirror" in GOLD:
            close(cq["mirror_symmetry"][b], GOLD[f"{key}_mirror"], "symmetry_score_mirror")
        if J == 15:
            close([cq["speed_mean"][b], cq["jerk_mean"][b]], GOLD[f"{key}_temporal"], "compute_temporal_metrics")
            close(cq["bone_cv_mean"][b], GOLD[f"{key}_bone_cv"], "compute_bone_length_cv")


@pytest.mark.parametrize("name", ec.FUSED)
def test_eval_fused_pose_restated(name):
    m = er.eval_fused_pose(*ec.fused_inputs(name))
    assert list(m) == list(GOLD[f"fused_{name}_keys"])
    assert ("Speed P95" in m) == (ec.CASES[name]["pred"].shape[0] >= 3)
    close(list(m.values()), GOLD[f"fused_{name}_values"], name)
    assert evaluate.format_fused_metrics(m).splitlines()[0] == evaluate.FUSED_METRICS_HEADER


def test_fused_metrics_text():
    for name in ec.FUSED:
        m = dict(zip((str(k) for k in GOLD[f"fused_{name}_keys"]), (float(v) for v in GOLD[f"fused_{name}_values"])))
        assert evaluate.format_fused_metrics(m) == str(GOLD[f"fused_{name}_text"])
    assert tuple(str(k) for k in GOLD["fused_clean_T21_J17_keys"]) == evaluate.FUSED_METRIC_KEYS == er.FUSED_METRIC_KEYS
    assert evaluate.format_fused_metrics({"Bone Length CV": 0.125}) == "Fused Pose Evaluation Metrics:\nBone Length CV           : 0.1250\n"


@pytest.mark.parametrize("group", list(ec.EVAL_CLIPS))
def test_evaluate_clips_weighting(group):
    names = ec.EVAL_CLIPS[group]
    preds, targets = [ec.CASES[n]["pred"] for n in names], [ec.CASES[n]["target"] for n in names]
    close(er.evaluate_clips(preds, targets, zero_root=0), GOLD[f"loop_{group}"], "evaluate_clips")
    # the product's weighting (torch ops, here on the host) on the restatement's per-clip numbers
    per = [er.pose_errors_clip(p, g, 0) for p, g in zip(preds, targets)]
    T = torch.tensor([p.shape[0] for p in preds], dtype=torch.float64)
    got = evaluate.weighted_mm(T, [torch.tensor([r[k] for r in per], dtype=torch.float64) for k in ("mpjpe", "p_mpjpe", "n_mpjpe", "mpjve")])
    close([float(v) for v in got], GOLD[f"loop_{group}"], "weighted_mm")
    # MPJVE is weighted by T_i, not T_i - 1: the other weighting gives another number
    other = sum((p.shape[0] - 1) * r["mpjve"] for p, r in zip(preds, per) if p.shape[0] > 1) / sum(p.shape[0] - 1 for p in preds) * 1000
    assert abs(other - GOLD[f"loop_{group}"][3]) > 1e-6


def test_rules_where_the_reference_raises_or_omits():
    # a frame without extent: no alignment, NaN and status 0, and the other frames keep theirs
    pe, _ = ec.restated("flat_T4_J17")
    assert list(pe["p_status"][0]) == [True, False, True, True] and pe["n_complete"][0] == 4
    assert np.isnan(pe["p_err"][0, 1]).all() and np.isnan(pe["p_R"][0, 1]).all() and np.isnan(pe["p_mpjpe_f"][0, 1])
    assert np.isfinite(pe["n_mpjpe_f"][0, 1]) and np.isfinite(pe["err"][0, 1]).all()
    # one joint has no extent in any frame
    pe, cq = ec.restated("clean_T3_J1")
    assert not pe["p_status"].any() and np.isnan(pe["p_mpjpe"][0]) and np.isfinite(pe["mpjpe"][0]) and pe["n_complete"][0] == 3
    # the mirrored frame: a proper rotation all the same, and the last singular value enters negated
    pe, _ = ec.restated("mirror_T4_J17")
    assert pe["p_status"].all() and np.allclose(np.linalg.det(pe["p_R"][0]), 1.0, atol=1e-12)
    c = ec.CASES["mirror_T4_J17"]
    s = er.singular_values(c["pred"][2:3], c["target"][2:3])[0]
    nX = np.sqrt(((c["target"][2] - c["target"][2].mean(0)) ** 2).sum())
    nY = np.sqrt(((c["pred"][2] - c["pred"][2].mean(0)) ** 2).sum())
    assert abs(pe["p_scale"][0, 2] - (s[0] + s[1] - s[2]) * nX / nY) <= 1e-12
    # incomplete frames have no Procrustes or N-MPJPE value, missing joints no error; a joint never seen has n = 0
    pe, cq = ec.restated("missing_T21_J17")
    assert not pe["p_status"][0, 5] and pe["n_valid_f"][0, 5] == 0 and np.isnan(pe["mpjpe_f"][0, 5])
    assert pe["joint_err_n"][0, 3] == 0 and np.isnan(pe["joint_err"][0, 3]).all() and pe["joint_err_n"][0, 4] == 1
    assert pe["n_complete"][0] == 0 and np.isnan(pe["p_mpjpe"][0]) and np.isnan(pe["n_mpjpe"][0])
    assert np.isnan(cq["speed_p95"][0]) and np.isnan(cq["accel_p95"][0]) and np.isfinite(cq["speed_mean"][0])
    pe0, _ = ec.restated("missing_zero_root_T21_J17")
    assert pe0["n_valid_f"][0, 2] == pe["n_valid_f"][0, 2] + 1          # the target's missing joint 12 is the origin there
    # the held ends and the gaps of np.interp give finite percentiles
    _, cq = ec.restated("gaps_T41_J15")
    assert np.isfinite(cq["speed_p95"][0]) and np.isfinite(cq["accel_p95"][0])
    # below 3 frames: no speed, jerk or percentile; no frame: nothing
    for name, n in (("clean_T0_J17", 0), ("clean_T1_J17", 1), ("clean_T2_J17", 2)):
        pe, cq = ec.restated(name)
        assert all(np.isnan(cq[k][0]) for k in ("speed_mean", "jerk_mean", "speed_p95", "accel_p95"))
        assert np.isnan(cq["mirror_symmetry"][0]) == (n == 0) and np.isnan(pe["mpjve"][0]) == (n < 2) and pe["n_vel"][0] == max(n - 1, 0) * 17
    # both parities of the medians
    assert {int(n) % 2 for name in ("clean_T4_J17", "clean_T21_J17", "missing_T21_J17") for n in ec.restated(name)[0]["joint_err_n"][0]} == {0, 1}
    # the ragged batch: nothing beyond a length is read
    pe, cq = ec.restated("ragged_B3_T41_J17")
    assert np.isnan(pe["err"][1, 18:]).all() and not pe["p_status"][1, 18:].any() and np.isnan(pe["mpjpe"][2]) and pe["n_err"][2] == 0
    assert np.isnan(cq["bone_len"][1, 18:]).all() and np.isfinite(cq["bone_cv_pooled"][:2]).all() and np.isnan(cq["bone_cv_pooled"][2])


def test_index_lists_are_the_reference_s():
    assert geometry.H36M_EDGES == er.H36M_EDGES and geometry.H36M_LR_PAIRS == er.H36M_LR_PAIRS
    assert geometry.H36M_LEFT_BONES == er.H36M_LEFT_BONES and geometry.H36M_RIGHT_BONES == er.H36M_RIGHT_BONES
    assert geometry.MHR70_15_EDGES == ec.MHR70_15_EDGES and geometry.MHR70_15_LR_PAIRS == ec.MHR70_15_LR_PAIRS
    ids = (1, 2, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 41, 62, 69)
    bones = ((69, 5), (5, 7), (7, 62), (69, 6), (6, 8), (8, 41), (69, 9), (9, 11), (11, 13), (69, 10), (10, 12), (12, 14), (9, 10), (5, 6))
    assert tuple((ids.index(a), ids.index(b)) for a, b in bones) == geometry.MHR70_15_EDGES
    assert set(geometry.MHR70_15_LEFT_BONES) | set(geometry.MHR70_15_RIGHT_BONES) == set(geometry.MHR70_15_EDGES[:12])


def test_argument_validation():
    lib = _lib.lib()
    z = C.c_void_p(0)
    i32 = lambda *v: (C.c_int32 * max(len(v), 1))(*v)      # noqa: E731

    def pe(clips, frames, joints, zero_root=-1):
        return lib.skimi_pose_errors(z, z, z, clips, frames, joints, zero_root, *([z] * 16), z)

    def cq(clips, frames, joints, edges=(), pairs=(), n_edges=None):
        return lib.skimi_clip_quality(z, z, clips, frames, joints, i32(*edges), len(edges) // 2 if n_edges is None else n_edges, i32(), 0,
                                      i32(), 0, i32(*pairs), len(pairs) // 2, z, 0, z, z, z, z)

    for args in ((1, 4, 0), (1, 4, 129), (-1, 4, 17), (1, -1, 17), (1, 2 ** 31, 17), (2 ** 31, 1, 17), (2 ** 20, 2 ** 12, 17)):
        assert pe(*args) == -1 and b"skimi_pose_errors" in lib.skimi_last_error(), args
        assert cq(*args) == -1 and b"skimi_clip_quality" in lib.skimi_last_error(), args
        assert lib.skimi_eval_workspace_bytes(*args) == 0
    assert pe(1, 4, 17, zero_root=17) == -1 and b"zero_root" in lib.skimi_last_error()
    assert pe(1, 4, 17, zero_root=-2) == -1
    assert pe(1, 4, 17) == -1 and b"NULL" in lib.skimi_last_error()          # sizes fine, no buffers
    assert pe(0, 4, 17) == 0 and cq(0, 4, 17) == 0                             # no clip: nothing to do
    assert cq(1, 4, 17, edges=(0, 17)) == -1 and b"edges[0][1] = 17" in lib.skimi_last_error()
    assert cq(1, 4, 17, pairs=(-1, 0)) == -1 and b"lr_pairs" in lib.skimi_last_error()
    assert cq(1, 4, 17, n_edges=129) == -1 and cq(1, 4, 17, pairs=(0, 0) * 65) == -1
    assert lib.skimi_eval_workspace_bytes(3, 41, 17) == 3 * 5 * 41 * 17 * 8
    # the wrappers: device tensors, matching shapes, known placements, short enough lists
    x = torch.zeros(4, 17, 3, dtype=torch.float64)
    with pytest.raises(_lib.SkimiError):
        geometry.pose_errors(x, x)
    with pytest.raises(_lib.SkimiError):
        geometry.clip_quality(x)
    assert evaluate.safe_pct_improvement(2.0, 1.0) == 50.0
    assert all(np.isnan(evaluate.safe_pct_improvement(a, b)) for a, b in ((0.0, 1.0), (float("nan"), 1.0), (1.0, float("inf"))))
    assert geometry.EVAL_LDS_ELEMS * 5 * 8 + 2048 <= 65536
