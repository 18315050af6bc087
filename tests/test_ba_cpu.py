"""CPU: the float64 restatement of the bundle adjustment (tests/ba_restated.py) against the reference's own losses
(bundle_adjustment/loss.py, via tests/golden/ba_losses.npz from tools/make_goldens.py ba) and torch.optim.Adam, and the
cfg parsing of the pipeline (multi_view_process.ba_settings, DESIGN §2 "BA")."""
import numpy as np
import pytest
import torch

import ba_restated as ref
from skiing_analysis_pytorch_amd import geometry
from skiing_analysis_pytorch_amd import multi_view_process as mv

INPUTS = ("K", "R", "t", "X", "x2d", "conf")


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(golden_dir / "ba_losses.npz")


def _close(got, want, rel):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape
    err = np.abs(got - want).max() / max(np.abs(want).max(), 1e-300)
    assert err <= rel, err


def _clip(gold, name):
    return {k: torch.tensor(gold[f"{name}_{k}"]) for k in INPUTS}


@pytest.mark.parametrize("name", ["a", "b"])
def test_terms_and_gradients_match_reference_losses(gold, name):
    a = _clip(gold, name)
    X, R, t = (a[k].clone().requires_grad_(True) for k in ("X", "R", "t"))
    tm = ref.terms(X, R, t, a["K"], a["x2d"], a["conf"])
    gX, gR, gt = torch.autograd.grad(tm[0] + tm[1] + tm[2] + tm[3] + tm[4], (X, R, t))
    for k in range(5):
        _close(tm[k].item(), gold[f"{name}_terms"][k], 1e-12)
    _close(gX.numpy(), gold[f"{name}_gX"], 1e-12)
    _close(gt.numpy(), gold[f"{name}_gt"], 1e-12)
    _close(gR.numpy(), gold[f"{name}_gR"], 1e-12)


@pytest.mark.parametrize("name", ["a", "b"])
def test_w_gradient_at_zero_is_the_skew_part_of_the_R_gradient(gold, name):
    a = _clip(gold, name)
    X, t = a["X"].clone().requires_grad_(True), a["t"].clone().requires_grad_(True)
    w = torch.zeros_like(a["t"]).requires_grad_(True)
    tm = ref.terms(X, ref.rodrigues(w) @ a["R"], t, a["K"], a["x2d"], a["conf"])
    (gw,) = torch.autograd.grad(tm.sum(), (w,))
    G, R0 = gold[f"{name}_gR"], gold[f"{name}_R"]
    M = G @ np.swapaxes(R0, -1, -2) - R0 @ np.swapaxes(G, -1, -2)
    vee = np.stack([M[..., 2, 1], M[..., 0, 2], M[..., 1, 0]], -1)
    assert np.isfinite(gw.numpy()).all()
    _close(gw.numpy(), vee, 1e-12)


def test_rodrigues_branches_meet():
    w = torch.tensor([[3e-5, -4e-5, 1e-5], [0.3, -0.2, 0.5], [0.0, 0.0, 0.0]], dtype=torch.float64)
    E = ref.rodrigues(w).numpy()
    assert np.allclose(E @ np.swapaxes(E, -1, -2), np.eye(3), atol=1e-15)
    # just above the threshold, the closed form equals the Taylor polynomial to rounding
    s = 1.0000001e-8
    wv = torch.tensor([[np.sqrt(s), 0.0, 0.0]], dtype=torch.float64)
    A_taylor = 1 - s / 6 + s * s / 120
    assert abs(ref.rodrigues(wv)[0, 2, 1].item() - A_taylor * np.sqrt(s)) < 1e-18


@pytest.mark.parametrize("mode", ["pose_only", "pose_cam_t", "full"])
def test_trajectory_matches_torch_adam_on_reference_losses(gold, mode):
    a = {k: gold[f"a_{k}"] for k in INPUTS}
    weights = dict(zip(ref.DEFAULT_WEIGHTS, gold["traj_weights"].tolist()))
    R, t, X, h = ref.run(a["K"], a["R"], a["t"], a["X"], a["x2d"], a["conf"], mode, int(gold["traj_steps"]),
                         float(gold["traj_lr"]), weights)
    for k, v in (("R", R), ("t", t), ("X", X), ("history", h)):
        _close(v.numpy(), gold[f"traj_{mode}_{k}"], 1e-12)
    if mode != "full":
        assert np.array_equal(R.numpy(), a["R"])
    if mode == "pose_only":
        assert np.array_equal(t.numpy(), a["t"])


def test_ba_settings_defaults_and_keys():
    modes, iters, lr, w = mv.ba_settings({})
    assert modes == ["pose_only", "pose_cam_t", "full"] and iters == 200 and lr == 1e-3 and w == {}
    cfg = {"bundle_adjustment": {"run_ba": True, "lr": 1e-2, "num_iters": 10000, "mode": "full",
                                 "ba_weight_reproj": 1.0, "ba_weight_smooth": 0.1, "ba_weight_bone_length": 0.1}}
    modes, iters, lr, w = mv.ba_settings(cfg)
    assert modes == ["full"] and iters == 10000 and lr == 1e-2
    assert w == {"ba_weight_reproj": 1.0, "ba_weight_smooth": 0.1, "ba_weight_bone_length": 0.1}
    # absent weight keys take the loss.py defaults, in the C-ABI order
    assert geometry.ba_weights(w) == [1.0, 0.1, 1e-2, 0.1, 1e-2]
    assert geometry.ba_weights(None) == [1.0, 1e-2, 1e-2, 1e-2, 1e-2]
    assert mv.ba_settings({"bundle_adjustment": {"mode": ["pose_cam_t", "pose_only"]}})[0] == ["pose_cam_t", "pose_only"]
    with pytest.raises(ValueError):
        mv.ba_settings({"bundle_adjustment": {"mode": "rotation_only"}})
    with pytest.raises(ValueError):
        geometry.ba_weights({"ba_weight_reprojection": 1.0})


def test_abi_errors_are_reported():
    """Bad sizes, an unknown mode and a short workspace come back through the return code and skimi_last_error
    (checked before anything touches the device)."""
    import ctypes

    from skiing_analysis_pytorch_amd import _lib

    lib = _lib.lib()
    d = 4096   # stands for a device pointer: never dereferenced on these paths

    def call(T=16, C=2, J=17, modes=(0,), placement=0, ws_bytes=1 << 30):
        m = (ctypes.c_int32 * len(modes))(*modes)
        return lib.skimi_bundle_adjust(d, d, d, d, d, d, T, C, J, m, len(modes), 10, 1e-3, 1.0, 1e-2, 1e-2, 1e-2, 1e-2,
                                       placement, d, d, d, None, d, ws_bytes, None)

    assert lib.skimi_ba_workspace_bytes(16, 2, 17, 3) == 3 * lib.skimi_ba_workspace_bytes(16, 2, 17, 1) > 0
    assert lib.skimi_ba_workspace_bytes(16, 9, 17, 1) == 0 and lib.skimi_ba_workspace_bytes(16, 2, 33, 1) == 0
    assert call(C=9) == -1 and b"C = 9" in lib.skimi_last_error()
    assert call(J=0) == -1 and call(T=0) == -1
    assert call(modes=(0, 3)) == -1 and b"unknown mode 3" in lib.skimi_last_error()
    assert call(placement=3) == -1 and b"placement" in lib.skimi_last_error()
    need = lib.skimi_ba_workspace_bytes(16, 2, 17, 1)
    assert call(placement=2, ws_bytes=need - 1) == -4 and b"workspace" in lib.skimi_last_error()
    assert call(T=4096, ws_bytes=lib.skimi_ba_workspace_bytes(4096, 2, 17, 1) - 1) == -4
    assert call(T=4096, placement=1) == -1 and b"does not fit in LDS" in lib.skimi_last_error()
