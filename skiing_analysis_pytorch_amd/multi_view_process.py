"""Counterpart of vggt/multi_view_process.py with the reference's signature:

    process_multi_view_video(left_video_path, left_pt_path, right_video_path, right_pt_path,
                             out_root, inference_output_path, cfg) -> Optional[Path]
                                                              (multi_view_process.py:68-76)

What it reproduces per time step (multi_view_process.py:133-309): left/right frame -> VGGT
(`CameraHead.reconstruct_from_frames`) -> person-centred world origin from the two point maps inside the
detector boxes (`extract_person_points`, :356-395) -> the right camera's 180-degree alignment (:204-217)
-> DLT triangulation of the 17 joints (`triangulate_one_frame`, vggt/triangulate.py:38-71), and at the
end the camera / joints NPZ of `save_camera_info` (vggt/save.py:84-110, called at :312-319).

With `cfg.infer.icp` true it also runs the reference's refinement of the right camera (:263-291): point-to-plane
ICP of the step's two world-point maps (`ICP_with_bbox`, :427-520; HIP kernels instead of Open3D,
geometry.icp_point_to_plane), the update of R[1] / t[1] (`apply_icp_update`) and a second triangulation; the NPZ
then holds the refined R, t and x3d, as the reference's does, with icp_refined=True.  The flag is off by default:
the arrays are then the pre-ICP quantities under the same keys, with icp_refined=False.  Parity with Open3D
itself is "unpinned" (DESIGN §2 "ICP": tie, eigensolver and non-finite-point rules of this build).

With `cfg.infer.ba` true it also runs the clip-level bundle adjustment that the reference defines but leaves
commented out (:321-353): after the all-gather, on rank 0, the gathered joints / R / t (after ICP when that is on),
the time-mean K (:543), the keypoints and their scores go through geometry.bundle_adjust (one HIP launch for every
mode of cfg.bundle_adjustment.mode, all three when it is absent, as the commented loop at :338 does) and the NPZ
gains ba_<mode>_x3d / _R / _t / _history.  `run_local_ba` is the function its caller names (:553-564), which the
reference never defines; its parity is unpinned beyond bundle_adjustment/loss.py (DESIGN §2 "BA").  The reference's
own `run_ba` key is not read: it ships true while the reference never runs BA.  Flag off (the default): the NPZ is
unchanged.

With `cfg.infer.device_origin` true the person origins come from the device (geometry.person_origin on the world
points the model call left in HBM; 16 numbers per step cross to the host instead of the dense maps, which
`reconstruct_batch(dense_to_host=False)` then never copies).  The kept point sets are the host path's; the origin is
their float64 mean where the host path sums in float32 (DESIGN §2 "Person origin").  With `cfg.infer.triage` true
geometry.triangulate_triage replaces the plain DLT: the NPZ gains reproj_err, x3d_clean, triage_keep, triage_report and
reproj_view_stats, and `raw_reprojection_error.txt` holds the per-step errors in the reference's layout (:244-250; its
`out_path` line names a panel image this build does not draw and is left out).  `cfg.triangulation.conf_thr` /
`.err_thresh_px` override post_triage_single's defaults (0.3, 2.0).  Both flags are off by default: the NPZ is unchanged.

With `cfg.infer.robust` true geometry.triangulate_robust runs as well (the consensus over the views of DESIGN §2 "Robust
triangulation"; with the reference's two cameras it can only accept or fail a joint, with more it recovers joints that
single views got wrong): the NPZ gains x3d_robust, x3d_robust_ok, robust_inlier_views, robust_rms_px and
robust_view_inlier_ratio.  `cfg.triangulation.inlier_px` (default: err_thresh_px), `.min_inliers` (2), `.refine_iters` (5)
and `.weighted` (false) are its parameters; x3d and the triage arrays are not touched.  Off by default: the NPZ is unchanged.

With `cfg.infer.undistort` true and `cfg.infer.calibration` naming a calibration file (one for both cameras, as the
reference's single K_dist, or a list of two; formats.load_calibration) the lens is taken out first: each call's source frames
are undistorted on the device (preprocess.undistort_images), the source-pixel keypoints are undistorted
(geometry.undistort_points) and the detector boxes become the bounding boxes of their four undistorted corners; the largest
resid_px is logged.  The NPZ keeps its keys.  Off by default, and with all-zero coefficients: exactly the run without it.

What it leaves out (out of scope): video decode (frames come from the `.pt` files, which
`prepare_dataset` can embed; the video paths only name the subject), PNG / matplotlib output, the camera cones and
sky mask of the scene GLB (its point cloud is written per step with `cfg.infer.scene_glb` true, default false:
`CameraHead.reconstruct_batch(scene=True)`) and the bundle adjustment's images (:566-627).  The time steps are independent: they go through the HIP model `steps_per_call` at a
time, sharded over ranks under torch.distributed, and the per-step joints are re-assembled with one
all-gather (parallel.py).
"""
from __future__ import annotations

import logging
from pathlib import Path
from typing import List, Optional

import numpy as np
import torch

from . import formats, fuse, geometry, parallel, preprocess
from .infer import CameraHead, cfg_get, lens_from_cfg, save_camera_info, undistort_detections

logger = logging.getLogger(__name__)

_R_ALIGN = np.array([[-1, 0, 0], [0, 1, 0], [0, 0, -1]], dtype=np.float64)   # multi_view_process.py:204-210


def extract_person_points(pointmap: np.ndarray, bbox, img_size) -> np.ndarray:
    """multi_view_process.py:356-395: the point-map pixels inside the detector box (box given in source
    pixels), finite, within 3 sigma of the median depth -> [N, 3]."""
    H_img, W_img = img_size
    H_pm, W_pm = pointmap.shape[:2]
    sx, sy = W_pm / W_img, H_pm / H_img
    x1, y1, x2, y2 = bbox
    x1, x2, y1, y2 = int(x1 * sx), int(x2 * sx), int(y1 * sy), int(y2 * sy)
    x1, x2 = np.clip(x1, 0, W_pm - 1), np.clip(x2, 0, W_pm)
    y1, y2 = np.clip(y1, 0, H_pm - 1), np.clip(y2, 0, H_pm)
    P = pointmap[y1:y2, x1:x2, :].reshape(-1, 3)
    P = P[np.isfinite(P).all(axis=1)]
    if len(P) > 0:
        z = P[:, 2]
        P = P[np.abs(z - np.median(z)) < 3.0 * np.std(z)]
    return P


def scale_bbox(bbox, source_size, target_size) -> List[float]:
    """multi_view_process.py:398-424"""
    (src_h, src_w), (tgt_h, tgt_w) = source_size, target_size
    sx, sy = tgt_w / src_w, tgt_h / src_h
    x1, y1, x2, y2 = bbox
    return [x1 * sx, y1 * sy, x2 * sx, y2 * sy]


def recenter_and_align(R: np.ndarray, t: np.ndarray, origin: np.ndarray):
    """multi_view_process.py:196-217 on copies: move the world origin onto the person
    (t_c += R_c @ origin), then turn the right camera by 180 degrees about y and mirror its x / z
    translation."""
    R, t = np.array(R, dtype=np.float64), np.array(t, dtype=np.float64)
    for cam in range(len(R)):
        t[cam] = t[cam] + R[cam] @ origin
    R[1] = _R_ALIGN @ R[1]
    t[1] = _R_ALIGN @ t[1]
    t[1][0] = -t[1][0]
    t[1][2] = -t[1][2]
    return R, t


def ICP_with_bbox(source_points, target_points, source_bbox, target_bbox):
    """multi_view_process.py:427-520: point-to-plane ICP of the whole source map onto the whole target map
    (the boxes are ignored: the reference's crop is commented out, :453-456) -> (aligned source [N, 3] =
    R_T p + t_T for every source point, float64 4x4 T).  Maps [H, W, 3] or [N, 3], device tensors or arrays;
    the ICP runs on the device (geometry.icp_point_to_plane with the reference's parameters: 0.05, 0.05, 200).
    Fewer than 50 valid points in either map: the unchanged source and eye(4) (:471-474)."""
    del source_bbox, target_bbox
    dev = torch.device("cuda", torch.cuda.current_device())
    src = source_points if isinstance(source_points, torch.Tensor) else torch.from_numpy(np.asarray(source_points, np.float32))
    tgt = target_points if isinstance(target_points, torch.Tensor) else torch.from_numpy(np.asarray(target_points, np.float32))
    src = src.to(dev).reshape(-1, 3)
    tgt = tgt.to(dev).reshape(-1, 3)
    T = geometry.icp_point_to_plane(src, tgt, 0.05, 0.05, 200).transformation
    P = src.cpu().numpy().astype(np.float64)
    return (T[:3, :3] @ P.T).T + T[:3, 3], T


def apply_icp_update(R: np.ndarray, t: np.ndarray, T: np.ndarray):
    """multi_view_process.py:271-275 on copies: R[1] = R_T R[1], t[1] = R_T t[1] + t_T.
    As in the reference, T is estimated between the world-point maps in VGGT's frame but applied to the camera
    AFTER the person recentring and the 180-degree turn of recenter_and_align (:196-217); that mismatch is the
    reference's and is reproduced, not fixed."""
    R, t = np.array(R, dtype=np.float64), np.array(t, dtype=np.float64)
    R_u, t_u = T[:3, :3], T[:3, 3]
    R[1] = R_u @ R[1]
    t[1] = R_u @ t[1] + t_u
    return R, t


def ba_settings(cfg):
    """cfg.bundle_adjustment -> (modes, num_iters, lr, weights) as the reference's caller reads them (:338, :560-561):
    `mode` a string or a list (absent: all three modes), num_iters 200 and lr 1e-3 when absent, and the ba_weight_*
    keys that are present (an absent one takes its loss.py default in geometry.bundle_adjust)."""
    mode = cfg_get(cfg, "bundle_adjustment.mode", None)
    if mode is None:
        modes = list(geometry.BA_MODES)
    elif isinstance(mode, str):
        modes = [mode]
    else:
        modes = [str(m) for m in mode]
    bad = [m for m in modes if m not in geometry.BA_MODES]
    if bad or not modes:
        raise ValueError(f"cfg.bundle_adjustment.mode: unknown modes {bad or modes}; known: {list(geometry.BA_MODES)}")
    num_iters = int(cfg_get(cfg, "bundle_adjustment.num_iters", 200))
    lr = float(cfg_get(cfg, "bundle_adjustment.lr", 1e-3))
    weights = {}
    for key in geometry.BA_WEIGHT_KEYS:
        v = cfg_get(cfg, f"bundle_adjustment.{key}", None)
        if v is not None:
            weights[key] = float(v)
    return modes, num_iters, lr, weights


def run_local_ba(K_torch, R_init_torch, t_init_torch, X3d_init_torch, x2d_torch, conf2d_torch, num_iters: int = 200,
                 lr: float = 1e-3, device="cuda", mode: str = "pose_only", weights=None):
    """The function the reference's bundle_adjustment() calls (:553-564) and never defines: K (C,3,3), R (T,C,3,3),
    t (T,C,3), X (T,J,3), x2d (T,C,J,2), conf (T,C,J) -> (R_opt, t_opt, X_opt, history) as float64 tensors on `device`
    (history [num_iters, 6]: total, then the five weighted terms).  One HIP launch (geometry.bundle_adjust)."""
    dev = torch.device(device)
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    with torch.cuda.device(dev):
        r = geometry.bundle_adjust(K_torch, R_init_torch, t_init_torch, X3d_init_torch, x2d_torch, conf2d_torch, modes=(mode,),
                                   num_iters=num_iters, lr=lr, weights=weights)[0]
    return r.R, r.t, r.X, r.history


def write_reprojection_errors(path: Path, view_stats: np.ndarray) -> None:
    """`raw_reprojection_error.txt` in the reference's layout (multi_view_process.py:244-250): per step a header line and
    the scalar entries of reproject_and_visualize's dict (vggt/reproject.py:334-341) in its order -- rmse_L, rmse_R,
    mean_err_L, ... max_err_R.  view_stats [T, 2, 4] (geometry.triangulate_triage)."""
    with open(path, "w") as f:
        for i, step in enumerate(view_stats):
            f.write(f"Frame {i:04d} Reprojection Error (in pixels):\n")
            for k, field in enumerate(geometry.VIEW_STAT_FIELDS):
                for v, side in enumerate("LR"):
                    f.write(f"  {field}_{side}: {float(step[v, k])}\n")


def _bbox_of(bboxes: np.ndarray, idx: int):
    b = bboxes[idx]
    return b if b.ndim == 1 else b[0]


def process_multi_view_video(left_video_path: Path, left_pt_path: Path, right_video_path: Path, right_pt_path: Path,
                             out_root: Path, inference_output_path: Path, cfg, camera_head: Optional[CameraHead] = None,
                             steps_per_call: int = 4) -> Optional[Path]:
    """Same arguments as the reference; `camera_head` (optional) supplies an already loaded model instead
    of `CameraHead(cfg, out_dir / "vggt_infer")` (offline there is no checkpoint URL: cfg.infer.ckpt_path
    names a local model.pt otherwise).  Returns the output directory."""
    left_video_path, right_video_path = Path(left_video_path), Path(right_video_path)
    out_root, inference_output_path = Path(out_root), Path(inference_output_path)
    subject = left_video_path.parent.name or "default"
    out_dir = out_root / "multi_view" / subject
    out_dir.mkdir(parents=True, exist_ok=True)
    inference_output_path.mkdir(parents=True, exist_ok=True)
    logger.info(f"[Run-MV] {left_video_path} & {right_video_path} -> {out_dir} | ")

    lk, ls, lb, _lbs, lf = formats.load_info(left_pt_path, video_file_path=left_video_path, assume_normalized=False)
    rk, rs, rb, _rbs, rf = formats.load_info(right_pt_path, video_file_path=right_video_path, assume_normalized=False)
    for frames_, pt_, vid_ in ((lf, left_pt_path, left_video_path), (rf, right_pt_path, right_video_path)):
        if frames_ is None:
            raise RuntimeError(f"{pt_} embeds no frames and {vid_} cannot be decoded here (formats.read_video_frames)")
    head = camera_head if camera_head is not None else CameraHead(cfg, out_dir / "vggt_infer")
    if head.outdir is None:
        head.outdir = out_dir / "vggt_infer"
    hflip = bool(cfg_get(cfg, "infer.hflip", False))
    # opt-in lens stage (DESIGN §2 "Lens distortion"): the detections are undistorted here, the frames chunk by chunk on the
    # device below; both belong to the sensor's own pixels, so they come before the mirror of hflip
    lens = lens_from_cfg(cfg, 2, (int(lf.shape[2]), int(lf.shape[1])))
    if lens is not None:
        lk, lb, worst_l, lost_l = undistort_detections(lk, lb, lens[0][0], lens[1][0], head.device)
        rk, rb, worst_r, lost_r = undistort_detections(rk, rb, lens[0][1], lens[1][1], head.device)
        logger.info(f"[Run-MV] lens: keypoints and boxes undistorted, largest resid_px {max(worst_l, worst_r):.3g}, "
                    f"{lost_l + lost_r} points lost to the inverse")
    if hflip:       # multi_view_process.py:116-127
        W0 = lf[0].shape[1]
        if lens is None:
            rf = torch.flip(rf, [2])
        rk = rk.copy()
        rk[..., 0] = W0 - rk[..., 0]
        rb = rb.copy()
        x1, x2 = rb[..., 0].copy(), rb[..., 2].copy()
        rb[..., 0], rb[..., 2] = W0 - x2, W0 - x1

    T = min(len(lf), len(rf))
    lo, hi, _T_pad = parallel.shard_range(T)
    source_size = tuple(lf.shape[1:3])
    icp = bool(cfg_get(cfg, "infer.icp", False))
    ba = bool(cfg_get(cfg, "infer.ba", False))
    device_origin = bool(cfg_get(cfg, "infer.device_origin", False))
    triage = bool(cfg_get(cfg, "infer.triage", False))
    conf_thr = float(cfg_get(cfg, "triangulation.conf_thr", 0.3))
    err_thresh_px = float(cfg_get(cfg, "triangulation.err_thresh_px", 2.0))
    robust = bool(cfg_get(cfg, "infer.robust", False))
    scene_glb = bool(cfg_get(cfg, "infer.scene_glb", False))   # opt-in: the reference's per-step scene GLB (vggt/save.py:58-73)
    inlier_px = float(cfg_get(cfg, "triangulation.inlier_px", err_thresh_px))
    min_inliers = int(cfg_get(cfg, "triangulation.min_inliers", 2))
    refine_iters = int(cfg_get(cfg, "triangulation.refine_iters", 5))
    weighted = bool(cfg_get(cfg, "triangulation.weighted", False))
    x3d_l, K_l, R_l, t_l, C_l = [], [], [], [], []
    triage_l = []   # per call: X_clean, err, keep (uint8), view_stats, report on the device
    robust_l = []   # per call: geometry.robust_launch's eight outputs on the device

    def step_frames(idx):
        """the [left, right] frames of the steps idx; with the lens stage on, undistorted on the device in one launch"""
        if lens is None:
            return [[lf[i], rf[i]] for i in idx]
        with torch.cuda.device(head.device):
            src = torch.stack([lf[idx], rf[idx]]).to(head.device)                    # [2, n, H, W, 3] raw sensor frames
            und = preprocess.undistort_images(src, lens[0], lens[1])
            if hflip:
                und[1] = torch.flip(und[1], [2])
        return [[und[0, b], und[1, b]] for b in range(len(idx))]

    for a in range(lo, hi, steps_per_call):
        idx = [min(i, T - 1) for i in range(a, min(a + steps_per_call, hi))]     # padded steps repeat the last one
        # a padded step (index >= T on the last ranks) is computed to keep the collective uniform, but does not
        # write frame_{T-1}/predictions.npz a second time
        write = [i < T for i in range(a, min(a + steps_per_call, hi))]
        if device_origin:
            recs = head.reconstruct_batch(idx, step_frames(idx), write=write, dense_to_host=False, scene=scene_glb)
            bx = np.stack([np.stack([_bbox_of(lb, i), _bbox_of(rb, i)]) for i in idx]).astype(np.float32)
            po = geometry.person_origin(head.last_world_points[:, :2], torch.from_numpy(bx).to(head.device), source_size)
            po_stats = po.stats.cpu().numpy()   # [n, 2, 8]: the only numbers of the dense maps that reach the host
        else:
            recs = head.reconstruct_batch(idx, step_frames(idx), write=write, scene=scene_glb)
        Ks, Rs, ts = [], [], []
        for b, (i, (_E, K_res, R, t, C, wp)) in enumerate(zip(idx, recs)):
            if device_origin:
                kept_both = po_stats[b, 0, 2] > 0 and po_stats[b, 1, 2] > 0
                origin = 0.5 * (po_stats[b, 0, 5:8] + po_stats[b, 1, 5:8]) if kept_both else np.zeros(3)
            else:
                pl = extract_person_points(wp[0], _bbox_of(lb, i), source_size)
                pr = extract_person_points(wp[1], _bbox_of(rb, i), source_size)
                origin = 0.5 * (pl.mean(axis=0) + pr.mean(axis=0)) if len(pl) and len(pr) else np.zeros(3)
            R2, t2 = recenter_and_align(R, t, origin)
            if icp:   # :263-275: ICP of view 0's map onto view 1's (the device copy of wp), then R[1], t[1] updated
                wpd = head.last_world_points[b]
                T_icp = geometry.icp_point_to_plane(wpd[0].reshape(-1, 3), wpd[1].reshape(-1, 3), 0.05, 0.05, 200).transformation
                R2, t2 = apply_icp_update(R2, t2, T_icp)
            Ks.append(np.stack(K_res[:2]))
            Rs.append(R2)
            ts.append(t2)
            C_l.append(np.asarray(C))
        Kd = torch.from_numpy(np.stack(Ks)).to(head.device, torch.float32)
        Rd = torch.from_numpy(np.stack(Rs)).to(head.device, torch.float32)
        td = torch.from_numpy(np.stack(ts)).to(head.device, torch.float32)
        kp = torch.from_numpy(np.stack([np.stack([lk[i], rk[i]]) for i in idx])).to(head.device, torch.float32)
        if triage or robust:
            conf = torch.from_numpy(np.stack([np.stack([ls[i], rs[i]]) for i in idx])).to(head.device, torch.float32)
        if robust:
            robust_l.append(geometry.robust_launch(Kd, Rd, td, kp, conf, conf_thr, inlier_px, min_inliers, refine_iters, weighted))
        if triage:
            X, Xc, err, _depth, keep, vs, rep = geometry.triage_launch(Kd, Rd, td, kp, conf, conf_thr, err_thresh_px)
            x3d_l.append(X)
            triage_l.append((Xc, err, keep, vs, rep))
        else:
            x3d_l.append(geometry.triangulate_joints(Kd, Rd, td, kp))          # [n, 17, 3] on the device
        K_l += Ks
        R_l += Rs
        t_l += ts
    # the path's ONE collective: joints + K + R + t + C of this rank's steps as one packed record per step
    # (no-op on one rank)
    dev = head.device
    todev = lambda lst: torch.from_numpy(np.stack(lst)).to(dev)   # noqa: E731
    parts = parallel.all_gather_packed(
        [torch.cat(x3d_l), todev(K_l), todev(R_l), todev(t_l), todev(C_l)]
        + ([torch.cat([r[k] for r in triage_l]) for k in range(5)] if triage else [])
        + ([torch.cat([r[k] for r in robust_l]) for k in range(8)] if robust else []), T)
    gathered = [a.cpu().numpy() for a in parts]
    x3d, Ka, Ra, ta, Ca = gathered[:5]
    # fuse/'s temporal smoothing of the gathered joints (BASELINE config 4; fuse/fuse.py:329-412); opt-in
    # infer.device_smooth: the same filter as one launch on the gathered device tensor (geometry.smooth_ema)
    if not cfg_get(cfg, "infer.smooth", True):
        x3d_smoothed = None
    elif cfg_get(cfg, "infer.device_smooth", False):
        with torch.cuda.device(dev):
            x3d_smoothed = geometry.smooth_ema(parts[0]).X.cpu().numpy()
    else:
        x3d_smoothed = fuse.temporal_smooth_ema(x3d.astype(np.float64))
    if parallel.world()[0] == 0:
        # the reference stores R, t and the joints AFTER its ICP update (multi_view_process.py:285-319); with
        # infer.icp off (the default) the arrays are the pre-ICP quantities under the same keys, icp_refined = False
        if not icp:
            logger.warning("[Run-MV] cameras / joints are written without the reference's Open3D ICP refinement (icp_refined=False)")
        extra = {"icp_refined": np.array(icp)} | ({"x3d_smoothed": x3d_smoothed} if x3d_smoothed is not None else {})
        if triage:
            x3d_clean, reproj_err, keep, view_stats, report = gathered[5:10]
            extra |= {"x3d_clean": x3d_clean, "reproj_err": reproj_err, "triage_keep": keep.astype(bool),
                      "triage_report": report, "reproj_view_stats": view_stats}
            write_reprojection_errors(out_dir / "raw_reprojection_error.txt", view_stats)
        if robust:
            xr, _err, inl, rms, _ok, xr_ok, ratio, _rep = gathered[-8:]
            extra |= {"x3d_robust": xr, "x3d_robust_ok": xr_ok, "robust_inlier_views": inl, "robust_rms_px": rms,
                      "robust_view_inlier_ratio": ratio}
        if ba:   # the reference's commented-out stage (:321-353), every mode in one launch
            modes, num_iters, lr, weights = ba_settings(cfg)
            x2d = np.stack([np.stack([lk[i], rk[i]]) for i in range(T)]).astype(np.float64)     # (T,C,J,2)
            conf = np.stack([np.stack([ls[i], rs[i]]) for i in range(T)]).astype(np.float64)    # (T,C,J)
            with torch.cuda.device(dev):
                res = geometry.bundle_adjust(Ka.astype(np.float64).mean(0), Ra, ta, x3d, x2d, conf, modes=modes,
                                             num_iters=num_iters, lr=lr, weights=weights)
            for r in res:
                extra[f"ba_{r.mode}_x3d"] = r.X.cpu().numpy()
                extra[f"ba_{r.mode}_R"] = r.R.cpu().numpy()
                extra[f"ba_{r.mode}_t"] = r.t.cpu().numpy()
                extra[f"ba_{r.mode}_history"] = r.history.cpu().numpy()
        save_camera_info(out_pt_path=inference_output_path / f"{subject}_multi_view_3d_info.npz",
                         all_frame_x3d=list(x3d), all_frame_camera_intrinsics=list(Ka), all_frame_R=list(Ra),
                         all_frame_t=list(ta), all_frame_C=list(Ca), extra=extra)
    return out_dir
