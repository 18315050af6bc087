"""Counterpart of VideoPose3D/run.py's entry point with the reference's signature:

    run_video_pose_3d(config, pt_path, out_dir, args) -> (prediction [T, 17, 3], depth)     (run.py:107)

The inference slice of that function, in its order: the clip's 2D keypoints from the `.pt` file
(CustomDataset, common/custom_dataset.py:106-151), screen normalisation (run.py:191-199), the lifter built
from `args` (:224-262) and loaded from `config.model.ckpt_path` (:284-289), UnchunkedGenerator padding +
flip TTA (:1070-1081, common/generators.py:216-239), `evaluate(return_predictions=True)` (:961-989),
`<out_dir>/<video_name>.npy` with the camera-space joints (:1086-1092), and the returned joints turned by
the dummy H36M camera and rebased in height (:1094-1108).  Left out: training, the
evaluation protocols, the rendered GIF.  The model call is the HIP `TemporalModel` (vp3d.py).

`solve_rt_from_3d` is the counterpart of VideoPose3D/slove_rt_from_3d.py: the lifter's 3D joints and both views' 2D
keypoints -> each camera's (R, t) and the pair's relative pose, on the device (geometry.resect_cameras).
`solve_rt_and_points` is that script's `--refine camera_points` mode: the joints are refined together with the cameras
(geometry.refine_cameras_points).  `solve_rt_from_essential` is its `--init essential` path: the right camera's pose relative to
the left one from the essential matrix of the 2D keypoints alone (geometry.essential_ransac), then the same refinement.

`process_video_3d` is the counterpart of VideoPose3D/main.py's process_video_3d: both views lifted, then fused per frame
without extrinsics on the device (geometry.fuse_h36m), and the fused joints written as the reference writes them;
`evaluate=True` adds its fused_metrics.txt (evaluate.eval_fused_pose on the device).
"""
from __future__ import annotations

from pathlib import Path

import numpy as np
import torch

from . import formats, geometry
from .infer import cfg_get
from .vp3d import (JOINTS_LEFT, JOINTS_RIGHT, KPS_LEFT, KPS_RIGHT, TemporalModel, merge_augmented,
                   normalize_screen_coordinates, pad_and_augment)

# common/custom_dataset.py:60-74: "Dummy camera parameters (taken from Human3.6M), only for visualization"
CUSTOM_CAMERA_ORIENTATION = np.array([0.1407056450843811, -0.1500701755285263, -0.755240797996521, 0.6223280429840088],
                                     dtype="float32")


def qrot(q: np.ndarray, v: np.ndarray) -> np.ndarray:
    """common/quaternion.py:10-24 (w first): v + 2 (w (q x v) + q x (q x v))"""
    qvec = q[..., 1:]
    uv = np.cross(qvec, v)
    uuv = np.cross(qvec, uv)
    return v + 2 * (q[..., :1] * uv + uuv)


def camera_to_world(X: np.ndarray, R: np.ndarray, t) -> np.ndarray:
    """common/camera.py:33-34"""
    return qrot(np.tile(R, (*X.shape[:-1], 1)), X) + t


def run_video_pose_3d(config, pt_path: Path, out_dir: Path, args, model_pos: TemporalModel = None):
    """Same arguments as the reference (`args` = the namespace of common/arguments.py; the fields read are
    architecture, causal, dropout, channels, dense, test_time_augmentation).  `model_pos` (optional) supplies
    an already loaded lifter instead of building one from `args` and `config.model.ckpt_path`."""
    pt_path, out_dir = Path(pt_path), Path(out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    pt = formats._load_pt(pt_path)
    video_name = pt["video_name"]
    H, W = (int(v) for v in pt["img_shape"])
    kps = pt["detectron2"]["keypoints"]
    kps = (kps.numpy() if isinstance(kps, torch.Tensor) else np.asarray(kps)).copy()
    # run.py:191-199: normalised in place, in the array's own dtype
    kps[..., :2] = normalize_screen_coordinates(kps[..., :2], w=W, h=H)

    if model_pos is None:
        filter_widths = [int(x) for x in str(getattr(args, "architecture", "3,3,3,3,3")).split(",")]
        model_pos = TemporalModel(kps.shape[-2], kps.shape[-1], 17, filter_widths=filter_widths,
                                  causal=bool(getattr(args, "causal", False)), dropout=getattr(args, "dropout", 0.25),
                                  channels=int(getattr(args, "channels", 1024)), dense=bool(getattr(args, "dense", False)))
        chk = cfg_get(config, "model.ckpt_path")
        if chk is None:
            raise RuntimeError("config.model.ckpt_path is not set (run.py:284-289)")
        checkpoint = torch.load(str(chk), map_location="cpu", weights_only=True)
        model_pos.load_state_dict(checkpoint["model_pos"])
    receptive_field = model_pos.receptive_field()
    pad = (receptive_field - 1) // 2
    causal_shift = pad if model_pos.causal else 0
    augment = bool(getattr(args, "test_time_augmentation", True))
    batch_2d = pad_and_augment(kps, pad, causal_shift, augment, KPS_LEFT, KPS_RIGHT)
    with torch.no_grad():
        pred = model_pos(torch.from_numpy(batch_2d.astype("float32")).cuda())
        if augment:
            pred = merge_augmented(pred, JOINTS_LEFT, JOINTS_RIGHT)
    prediction = pred.squeeze(0).cpu().numpy()
    # Predictions are in camera space (run.py:1086-1092)
    np.save(out_dir / (str(video_name) + ".npy"), prediction)
    # run.py:1094-1108: invert the (dummy) camera rotation, rebase the height
    prediction = camera_to_world(prediction, R=CUSTOM_CAMERA_ORIENTATION, t=0)
    prediction[:, :, 2] -= np.min(prediction[:, :, 2])
    depth = pt.get("depth", None)
    if isinstance(depth, torch.Tensor):
        depth = depth.squeeze()
    return prediction, depth


def process_video_3d(config, left_path: Path, right_path: Path, out_dir: Path, npy_dir: Path, args, model_pos: TemporalModel = None,
                     analyze: bool = False, evaluate: bool = False):
    """VideoPose3D/main.py:33-103 process_video_3d without its GIF (eval_fused_pose: evaluate=True): both views' clips are lifted
    (run_video_pose_3d into <out_dir>/videopose3d/left and /right) and fused frame by frame with the reference's settings
    (tau = 0.06, allow_scale = False, mirror_right_x = False) -- here as ONE geometry.fuse_h36m launch over the clip, in
    float64, where the reference loops over the frames on the host.  The fused, left and right joints are written with
    formats.save_3d_joints to "<npy_dir>_fused_keypoints.npy" (:85-90).  The clips are cut to the shorter one (the reference
    indexes the right clip by the left one's length and would raise).  `args` is passed in where the reference parses the
    command line (:41).  -> (fused [T, 17, 3] float64 on the device, geometry.FuseH36MResult with the per-frame R, t, s,
    diagnostics, status, mean_gain and bad_frames on the device).  analyze=True adds the skiing analysis of the fused clip
    (angle/main.py's process_person without its pictures): the clip stays on the device, goes through geometry.kinematics
    with the Human3.6M layout (angle.H36M_17, y pointing down as the lifter's camera frame has it) and the reference's CSV
    files land in <out_dir>/angle.  evaluate=True adds the reference's last step (:92-102): evaluate.eval_fused_pose of the
    left, right and fused clips on the device (geometry.pose_errors + geometry.clip_quality, one read-back) written to
    <out_dir>/fused_metrics.txt in the reference's format.  With analyze and evaluate off nothing else changes: every file is
    bitwise what it was."""
    out_dir = Path(out_dir)
    left, _ = run_video_pose_3d(config, left_path, out_dir / "videopose3d" / "left", args, model_pos=model_pos)
    right, _ = run_video_pose_3d(config, right_path, out_dir / "videopose3d" / "right", args, model_pos=model_pos)
    T = min(left.shape[0], right.shape[0])
    left, right = left[:T], right[:T]
    dev = torch.device("cuda", torch.cuda.current_device())
    res = geometry.fuse_h36m(torch.from_numpy(np.ascontiguousarray(left)).to(dev, torch.float64),
                             torch.from_numpy(np.ascontiguousarray(right)).to(dev, torch.float64), tau=0.06, allow_scale=False,
                             mirror_right_x=False)
    formats.save_3d_joints(res.fused.cpu().numpy(), left, right, Path(str(npy_dir) + "_fused_keypoints.npy"))
    if analyze:
        from . import angle

        angle.write_person(angle.analysis_from(geometry.kinematics(res.fused, layout=angle.H36M_17)), out_dir / "angle")
    if evaluate:
        from . import evaluate as ev

        ev.write_fused_metrics(out_dir / "fused_metrics.txt", ev.eval_fused_pose(left, right, res.fused))
    return res.fused, res


def _rt_inputs(X3d, x2d_left, x2d_right, conf_left, conf_right, K_left, K_right, huber, min_conf):
    """the script's inputs on the device -> X [N,3], x2d [2,N,2], K [2,3,3] | None, keywords (conf, loss, f_scale, min_conf)"""
    dev = torch.device("cuda", torch.cuda.current_device())

    def up(a, last):       # to_Nx (:47-63) + upload
        a = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.asarray(a))
        if a.dim() not in (2, 3) if last else a.dim() not in (1, 2):
            raise ValueError(f"Bad shape {tuple(a.shape)}")
        return (a.reshape(-1, last) if last else a.reshape(-1)).to(dev, torch.float64)

    X = up(X3d, 3)
    x2d = torch.stack([up(x2d_left, 2), up(x2d_right, 2)])
    conf = None
    if conf_left is not None or conf_right is not None:
        conf = torch.stack([torch.ones_like(X[:, 0]) if c is None else up(c, 0) for c in (conf_left, conf_right)])
    kw = dict(conf=conf, loss="soft_l1" if huber > 0 else "linear", f_scale=max(float(huber), 1.0), min_conf=float(min_conf))
    Ks = [None if k is None else up(k, 3).reshape(3, 3) for k in (K_left, K_right)]
    if Ks[0] is None and Ks[1] is None:
        K = None
    elif Ks[0] is None or Ks[1] is None:
        # one K given: the other is the one a call without K infers for that view from the points rule 1 keeps.  That is a
        # second launch (mask, K, start and one linearisation of both views: one pass set over the clip) spent so that the
        # mask and the two-pass std stay the kernel's own and are not restated here
        K_inf = geometry.resect_cameras(X, x2d, max_evals=1, **kw).K[0]
        K = torch.stack([K_inf[v] if k is None else k for v, k in enumerate(Ks)])
    else:
        K = torch.stack(Ks)
    return X, x2d, K, kw


RT_KEYS = ("RL", "tL", "RR", "tR", "R_rel", "t_rel", "K_L", "K_R", "mean_err_L", "median_err_L", "mean_err_R", "median_err_R",
           "success", "n_points")      # slove_rt_from_3d.py:263-271


def solve_rt_from_3d(X3d, x2d_left, x2d_right, conf_left=None, conf_right=None, K_left=None, K_right=None, refine="camera",
                     huber=0.0, min_conf=0.0, out=None, init="pnp"):
    """VideoPose3D/slove_rt_from_3d.py's main with its command-line arguments as keywords: X3d (N,3) | (T,J,3), x2d_*
    (N,2) | (T,J,2), conf_* (N,) | (T,J), K_* (3,3), host arrays or tensors -> dict with the reference's npz keys (host
    values), written to `out` when given.  One pose per view over the whole clip; loss soft_l1 with f_scale = max(huber, 1)
    when huber > 0 (:237, :244); an absent K is inferred from that view's masked keypoints (:65-73).  The start is this
    build's DLT resection where the reference calls cv2's EPnP, and refine="none" returns it.  init="essential" is
    solve_rt_from_essential and refine="camera_points" is solve_rt_and_points, entry points of their own."""
    if init == "essential":
        raise NotImplementedError('init="essential" (the start comes from the 2D keypoints alone and K is required) is not a mode of '
                                  'solve_rt_from_3d, DESIGN §2 "Essential matrix": call solve_rt_from_essential')
    if refine == "camera_points":
        raise NotImplementedError('refine="camera_points" (the views no longer decouple) is not a mode of solve_rt_from_3d, DESIGN §2 '
                                  '"Resection": call solve_rt_and_points')
    if init != "pnp" or refine not in ("none", "camera"):
        raise ValueError(f"solve_rt_from_3d: init {init!r} / refine {refine!r}; known: pnp; none, camera")
    X, x2d, K, kw = _rt_inputs(X3d, x2d_left, x2d_right, conf_left, conf_right, K_left, K_right, huber, min_conf)
    r = geometry.resect_cameras(X, x2d, K=K, max_evals=1 if refine == "none" else 200, **kw)
    R, t, err = r.R[0].cpu().numpy(), r.t[0].cpu().numpy(), r.err.cpu().numpy()
    used = ~np.isnan(err)
    med = [float(np.median(err[v][used[v]])) if used[v].any() else float("nan") for v in range(2)]
    ok = bool(r.success[0].all()) if refine != "none" else bool(np.isfinite(R).all() and np.isfinite(t).all())
    res = dict(RL=R[0], tL=t[0], RR=R[1], tR=t[1], R_rel=r.R_rel[0, 1].cpu().numpy(), t_rel=r.t_rel[0, 1].cpu().numpy(),
               K_L=r.K[0, 0].cpu().numpy(), K_R=r.K[0, 1].cpu().numpy(), mean_err_L=float(r.mean_err[0, 0]), median_err_L=med[0],
               mean_err_R=float(r.mean_err[0, 1]), median_err_R=med[1], success=int(ok), n_points=int(r.n_points[0, 0]))
    if out is not None:
        Path(out).parent.mkdir(parents=True, exist_ok=True)
        np.savez(out, **res)
    return res


def solve_rt_and_points(X3d, x2d_left, x2d_right, conf_left=None, conf_right=None, K_left=None, K_right=None, lambda_x=0.0,
                        huber=0.0, min_conf=0.0, out=None):
    """VideoPose3D/slove_rt_from_3d.py --init pnp --refine camera_points with its arguments as keywords: inputs as
    solve_rt_from_3d takes them -> dict with RT_KEYS plus `X_opt` (N,3) float64, the refined joints (a point the mask drops
    keeps its input value), and `mask` (N,) bool, the points rule 1 keeps (from the inputs alone: it is what it is
    when the solve fails, and sums to n_points); written to `out` when given.  Both cameras and the
    masked joints are refined together from the DLT start and X3d itself (:236), under the prior lambda_x ||X - X3d||^2
    (:159-161); with lambda_x = 0, the reference's default, the result is determined up to a similarity only.  The
    reference computes X_opt (:247) and takes its errors there (:257-260) but forgets to save it (:263-271); this build
    returns and writes it.  The errors are those of the final cameras at X_opt."""
    X, x2d, K, kw = _rt_inputs(X3d, x2d_left, x2d_right, conf_left, conf_right, K_left, K_right, huber, min_conf)
    r = geometry.refine_cameras_points(X, x2d, K=K, lambda_x=float(lambda_x), max_evals=200, **kw)
    R, t, err = r.R[0].cpu().numpy(), r.t[0].cpu().numpy(), r.err.cpu().numpy()
    used = ~np.isnan(err)
    med = [float(np.median(err[v][used[v]])) if used[v].any() else float("nan") for v in range(2)]
    mask = torch.isfinite(X).all(dim=1) & torch.isfinite(x2d).all(dim=2).all(dim=0)           # DESIGN rule 1
    if kw["conf"] is not None:
        w = torch.where(torch.isfinite(kw["conf"]), kw["conf"].clamp(0.0, 1.0), torch.zeros_like(kw["conf"]))
        mask = mask & (w >= kw["min_conf"]).all(dim=0)
    res = dict(RL=R[0], tL=t[0], RR=R[1], tR=t[1], R_rel=r.R_rel[0, 1].cpu().numpy(), t_rel=r.t_rel[0, 1].cpu().numpy(),
               K_L=r.K[0, 0].cpu().numpy(), K_R=r.K[0, 1].cpu().numpy(), mean_err_L=float(r.mean_err[0, 0]), median_err_L=med[0],
               mean_err_R=float(r.mean_err[0, 1]), median_err_R=med[1], success=int(bool(r.success[0])),
               n_points=int(r.n_points[0]), X_opt=r.X_opt.cpu().numpy(), mask=mask.cpu().numpy())
    if out is not None:
        Path(out).parent.mkdir(parents=True, exist_ok=True)
        np.savez(out, **res)
    return res


def solve_rt_from_essential(X3d, x2d_left, x2d_right, conf_left=None, conf_right=None, K_left=None, K_right=None, refine="camera",
                            huber=0.0, min_conf=0.0, out=None, hypotheses=1024, seed=0, threshold=1.0):
    """VideoPose3D/slove_rt_from_3d.py --init essential with its arguments as keywords: inputs as solve_rt_from_3d takes
    them, K_left and K_right required (the script's usage says so; each view is normalised through its own K where the
    script passes K_L for both) -> dict with RT_KEYS plus `inliers` (N,) bool, the keypoint pairs the winning essential
    matrix keeps; written to `out` when given.  The left camera starts at the identity and the right one at (R, t^) of
    geometry.essential_ransac over the points rule 1 of the resection keeps (:227-232; ||t^|| = 1: the scale is unknown,
    and the refinement against X3d supplies it); refine="none" returns that start with its errors, refine="camera" hands it
    to geometry.resect_cameras(R0=, t0=).  No essential matrix (fewer than 5 usable pairs): RuntimeError, as the script."""
    if refine == "camera_points":
        raise NotImplementedError('refine="camera_points" is not a mode of solve_rt_from_essential, DESIGN §2 "Essential matrix": '
                                  'call solve_rt_and_points')
    if refine not in ("none", "camera"):
        raise ValueError(f"solve_rt_from_essential: refine {refine!r}; known: none, camera")
    if K_left is None or K_right is None:
        raise ValueError("solve_rt_from_essential: K_left and K_right are required (slove_rt_from_3d.py: --init essential needs K)")
    X, x2d, K, kw = _rt_inputs(X3d, x2d_left, x2d_right, conf_left, conf_right, K_left, K_right, huber, min_conf)
    # the script masks first (:97-101) and estimates E on what is left: a point without a finite X3d takes no part
    nan = torch.full_like(x2d, float("nan"))
    e = geometry.essential_ransac(torch.where(torch.isfinite(X).all(dim=1)[None, :, None], x2d, nan), K, conf=kw["conf"],
                                  min_conf=kw["min_conf"], threshold=threshold, hypotheses=hypotheses, seed=seed)
    if not bool(e.success[0]):
        raise RuntimeError("findEssentialMat failed")
    R0 = torch.stack([torch.eye(3, dtype=torch.float64, device=X.device), e.R[0]])[None]
    t0 = torch.stack([torch.zeros(3, dtype=torch.float64, device=X.device), e.t[0]])[None]
    r = geometry.resect_cameras(X, x2d, K=K, R0=R0, t0=t0, max_evals=1 if refine == "none" else 200, **kw)
    R, t, err = r.R[0].cpu().numpy(), r.t[0].cpu().numpy(), r.err.cpu().numpy()
    used = ~np.isnan(err)
    med = [float(np.median(err[v][used[v]])) if used[v].any() else float("nan") for v in range(2)]
    ok = bool(r.success[0].all()) if refine != "none" else bool(np.isfinite(R).all() and np.isfinite(t).all())
    res = dict(RL=R[0], tL=t[0], RR=R[1], tR=t[1], R_rel=r.R_rel[0, 1].cpu().numpy(), t_rel=r.t_rel[0, 1].cpu().numpy(),
               K_L=r.K[0, 0].cpu().numpy(), K_R=r.K[0, 1].cpu().numpy(), mean_err_L=float(r.mean_err[0, 0]), median_err_L=med[0],
               mean_err_R=float(r.mean_err[0, 1]), median_err_R=med[1], success=int(ok), n_points=int(r.n_points[0, 0]),
               inliers=e.inliers.bool().cpu().numpy())
    if out is not None:
        Path(out).parent.mkdir(parents=True, exist_ok=True)
        np.savez(out, **res)
    return res


# ---- fuse/main_unity.py run_batch for one camera group ---------------------------------------------------------------------
GROUP_TARGET_IDS = (1, 2, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 41, 62, 69)      # fuse/main_unity.py: TARGET_IDS
_CAMERA_SUFFIXES = ("_sam_3d_body_outputs", "_sam_3d_body_output", "_outputs")


def camera_name_from_path(path) -> str:
    """fuse/main_unity.py:62-68: the file's stem without the first of the known output suffixes it ends with"""
    stem = Path(path).stem
    for suffix in _CAMERA_SUFFIXES:
        if stem.endswith(suffix):
            return stem[: -len(suffix)]
    return stem


def load_camera_sequence(path, target_ids=GROUP_TARGET_IDS):
    """fuse/main_unity.py:80-95 in array form: an .npz with the per-frame records under the key `outputs` (else under its
    first key), each with pred_keypoints_2d [N, 2] and pred_keypoints_3d [N, 3] -> (p2d [T, J, 2], p3d [T, J, 3]) float64,
    the rows `target_ids` of every frame."""
    ids = list(target_ids)
    with np.load(path, allow_pickle=True) as data:
        frames = data["outputs" if "outputs" in data.files else data.files[0]]
        p2d = np.full((len(frames), len(ids), 2), np.nan)
        p3d = np.full((len(frames), len(ids), 3), np.nan)
        for t, frame in enumerate(frames):
            p2d[t] = np.asarray(frame["pred_keypoints_2d"], dtype=np.float64)[ids]
            p3d[t] = np.asarray(frame["pred_keypoints_3d"], dtype=np.float64)[ids]
    return p2d, p3d


def group_inputs(inputs, names=None, target_ids=None):
    """V paths or V (p2d, p3d) array pairs -> (names, U [V, T, J, 2], X [V, T, J, 3]) on the host, every sequence cut to the
    shortest one (fuse/main_unity.py:104).  Paths are named by camera_name_from_path, array pairs cam0, cam1, ..."""
    ids = GROUP_TARGET_IDS if target_ids is None else tuple(target_ids)
    seqs, auto = [], []
    for i, item in enumerate(inputs):
        if isinstance(item, (str, Path)):
            seqs.append(load_camera_sequence(item, ids))
            auto.append(camera_name_from_path(item))
        else:
            p2d, p3d = (np.asarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=np.float64) for a in item)
            seqs.append((p2d, p3d))
            auto.append(f"cam{i}")
    names = auto if names is None else [str(n) for n in names]
    if len(names) != len(seqs):
        raise ValueError(f"fuse_camera_group: {len(names)} names for {len(seqs)} cameras")
    if len(seqs) < 2:
        raise ValueError("fuse_camera_group: a group needs at least two cameras")
    T = min(min(len(p2d), len(p3d)) for p2d, p3d in seqs)
    U, X = np.stack([p2d[:T] for p2d, _ in seqs]), np.stack([p3d[:T] for _, p3d in seqs])
    if X.ndim != 4 or X.shape[3] != 3 or U.shape != X.shape[:3] + (2,):
        raise ValueError(f"fuse_camera_group: need p3d [T, J, 3] and p2d [T, J, 2] per camera, got {list(X.shape)}, {list(U.shape)}")
    return names, U, X


def save_group(out_dir, names, pairs, smoothed, fused=None):
    """fuse/save.py for every pair: <a>__<b>_smoothed.npy (and _fused.npy when `fused` is given), [T, J, 3] float64 with NaN
    for missing joints -> the paths written"""
    out_dir = Path(out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    written = []
    for p, (a, b) in enumerate(pairs):
        stem = f"{names[int(a)]}__{names[int(b)]}"
        for kind, arr in (("fused", fused), ("smoothed", smoothed)):
            if arr is None:
                continue
            path = out_dir / f"{stem}_{kind}.npy"
            np.save(path, np.ascontiguousarray(arr[p], dtype=np.float64))
            written.append(path)
    return written


def _fuse_camera_group(layer, dev, inputs, out_dir, names, target_ids, fuse_kw, ema_kw, quality, size, edges, save_raw_fused):
    """fuse_camera_group's body with the module the device calls are taken from (`layer`: geometry), the device the clips go
    to and the keywords of the two calls"""
    ids = GROUP_TARGET_IDS if target_ids is None else tuple(target_ids)
    names, U, X = group_inputs(inputs, names, ids)
    if X.shape[1] == 0:
        raise ValueError("fuse_camera_group: the shortest sequence is empty; nothing to save")
    Xd, Ud = torch.from_numpy(X).to(dev), torch.from_numpy(U).to(dev)
    if isinstance(quality, str) and quality == "nogt":
        from . import skeleton
        if size is None:
            raise ValueError('fuse_camera_group: quality="nogt" needs size=(width, height)')
        quality = layer.joint_quality(Xd, Ud, edges=skeleton.MHR70_15_EDGES if edges is None else edges, size=size).q
    elif not isinstance(quality, str):
        quality = (quality if isinstance(quality, torch.Tensor) else torch.as_tensor(np.asarray(quality, dtype=np.float64))).to(dev)
    g = layer.fuse_group(Xd, Ud, quality=quality, **fuse_kw)
    sm = layer.smooth_ema(g.fused, target_ids=ids if len(ids) == X.shape[2] else None, **ema_kw)
    pairs, fused, smoothed = g.pairs.cpu().numpy(), g.fused.cpu().numpy(), sm.X.cpu().numpy()
    paths = save_group(out_dir, names, pairs, smoothed, fused if save_raw_fused else None)
    return dict(names=names, pairs=pairs, fused=fused, smoothed=smoothed, paths=paths)


def fuse_camera_group(inputs, out_dir, *, names=None, sigma_px=12.0, sigma_3d=0.08, alpha=0.7, adaptive_smooth=True,
                      smooth_alpha_min=0.45, smooth_alpha_max=0.92, smooth_speed_gain=0.25, save_raw_fused=False,
                      quality="confidence", target_ids=None, root_idx=14, left_hip_idx=11, right_hip_idx=12, left_shoulder_idx=5,
                      right_shoulder_idx=6, scale_mode="hip", min_points=8, align=False, size=None, edges=None):
    """fuse/main_unity.py's run_batch for one camera group: `inputs` are V .npz paths (the reference's layout, see
    load_camera_sequence) or V (p2d, p3d) array pairs; every pair of cameras is fused (one geometry.fuse_group call), every
    fused clip smoothed (one batched geometry.smooth_ema call) and written as fuse/save.py does, <a>__<b>_smoothed.npy and,
    with save_raw_fused, <a>__<b>_fused.npy -> dict(names, pairs, fused, smoothed (host arrays [P, T, J, 3]), paths).
    The five key joints default to the reference's 14, 11, 12, 5, 6: these are POSITIONS in the 15-joint array (what the
    reference's dict-to-array conversion makes of its IDX_* constants), not MHR-70 ids.  quality: "confidence" (the
    reference), "nogt" (geometry.joint_quality on `edges`, default skeleton.MHR70_15_EDGES, with the image `size`) or a [V, T,
    J] array of qualities.  target_ids: the joint rows taken from a file and the ids the EMA's per-joint factors go by."""
    fuse_kw = dict(root_idx=root_idx, left_hip_idx=left_hip_idx, right_hip_idx=right_hip_idx, left_shoulder_idx=left_shoulder_idx,
                   right_shoulder_idx=right_shoulder_idx, sigma_px=sigma_px, sigma_3d=sigma_3d, scale_mode=scale_mode,
                   min_points=min_points, align=align)
    ema_kw = dict(alpha=alpha, adaptive=adaptive_smooth, alpha_min=smooth_alpha_min, alpha_max=smooth_alpha_max,
                  speed_gain=smooth_speed_gain)
    return _fuse_camera_group(geometry, torch.device("cuda", torch.cuda.current_device()), inputs, out_dir, names, target_ids,
                              fuse_kw, ema_kw, quality, size, edges, save_raw_fused)
