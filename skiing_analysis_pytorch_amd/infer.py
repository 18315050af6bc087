"""Counterparts of the reference's VGGT entry points, with the same signatures and return values
but none of the per-frame PNG / matplotlib I/O (out of scope: SURVEY §8; the per-step GLB point cloud is
opt-in: `predictions_to_glb_points`, `CameraHead.reconstruct_batch(scene=True)`):

    load_and_preprocess_images        vggt/load.py:38-183
    CameraHead                        vggt/vggt/infer.py:46-215   (run_vggt, reconstruct_from_frames, ...)
    predictions_to_glb_points         vggt/visual_util.py:39-236  (the point cloud of predictions_to_glb)
    process_multi_view_clip           the hot loop of vggt/multi_view_process.py:133-309
    process_single_view_clip          vggt/single_view_process.py:130-170

The model call is the HIP VGGT (skiing_analysis_pytorch_amd.vggt.VGGT); pose decoding,
depth unprojection and DLT triangulation also run on device (geometry.py); only the final small
arrays cross to the host.  Time steps of a clip are independent, so under torch.distributed they
are sharded across ranks and the per-step 3D joints are re-assembled with ONE all-gather
(parallel.py).
"""
from __future__ import annotations

from pathlib import Path
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import geometry, parallel
from ._lib import PREC_BF16, PREC_BF16X3
from .vggt import VGGT
from .weights import VGGTConfig


def load_and_preprocess_images(image_list: Sequence, mode: str = "crop", device=None) -> torch.Tensor:
    """vggt/load.py:38-183.  image_list: HWC uint8 tensors / arrays.  Width -> 518 (bicubic, PIL),
    height -> round(h*518/w/14)*14, centre-crop heights > 518 ("crop") or pad to 518x518 with
    white ("pad").  Returns [N, 3, H, W] float32 in [0, 1] on the host (as the reference), or, with
    `device="cuda"`, computed on and left in GPU memory (preprocess.py: Pillow's resampler as HIP
    kernels, bit-identical to the host path)."""
    if device is not None and torch.device(device).type == "cuda":
        from .preprocess import load_and_preprocess_images_device
        return load_and_preprocess_images_device(image_list, mode, device)
    from PIL import Image

    if len(image_list) == 0:
        raise ValueError("At least 1 image is required")
    if mode not in ["crop", "pad"]:
        raise ValueError("Mode must be either 'crop' or 'pad'")
    images, shapes = [], set()
    target = 518
    for im in image_list:
        arr = im.numpy() if isinstance(im, torch.Tensor) else np.asarray(im)
        img = Image.fromarray(arr)
        if img.mode == "RGBA":
            bg = Image.new("RGBA", img.size, (255, 255, 255, 255))
            img = Image.alpha_composite(bg, img)
        img = img.convert("RGB")
        width, height = img.size
        if mode == "pad":
            if width >= height:
                new_w = target
                new_h = round(height * (new_w / width) / 14) * 14
            else:
                new_h = target
                new_w = round(width * (new_h / height) / 14) * 14
        else:
            new_w = target
            new_h = round(height * (new_w / width) / 14) * 14
        img = img.resize((new_w, new_h), Image.Resampling.BICUBIC)
        t = torch.from_numpy(np.asarray(img, dtype=np.uint8).copy()).permute(2, 0, 1).to(torch.float32) / 255.0
        if mode == "crop" and new_h > target:
            y0 = (new_h - target) // 2
            t = t[:, y0:y0 + target, :]
        if mode == "pad":
            hp, wp = target - t.shape[1], target - t.shape[2]
            if hp > 0 or wp > 0:
                t = torch.nn.functional.pad(t, (wp // 2, wp - wp // 2, hp // 2, hp - hp // 2), mode="constant", value=1.0)
        shapes.add((t.shape[1], t.shape[2]))
        images.append(t)
    if len(shapes) > 1:
        mh, mw = max(s[0] for s in shapes), max(s[1] for s in shapes)
        padded = []
        for t in images:
            hp, wp = mh - t.shape[1], mw - t.shape[2]
            if hp > 0 or wp > 0:
                t = torch.nn.functional.pad(t, (wp // 2, wp - wp // 2, hp // 2, hp - hp // 2), mode="constant", value=1.0)
            padded.append(t)
        images = padded
    return torch.stack(images)


_MISSING = object()


def cfg_get(cfg, dotted: str, default=None):
    """`cfg.a.b` / `cfg["a"]["b"]` / `cfg.a.get("b", default)` of the reference's OmegaConf configs
    (configs/vggt.yaml), for any mapping- or attribute-style object (omegaconf itself is not needed)."""
    cur = cfg
    for key in dotted.split("."):
        if cur is None:
            return default
        nxt = _MISSING
        if hasattr(cur, "get"):
            try:
                nxt = cur.get(key, _MISSING)
            except TypeError:
                nxt = _MISSING
        if nxt is _MISSING:
            nxt = getattr(cur, key, _MISSING)
        if nxt is _MISSING:
            return default
        cur = nxt
    return cur


def lens_from_cfg(cfg, cameras: int, frame_size):
    """The lens stage of the entry points: None unless cfg.infer.undistort is true (default false), else (K [cameras, 3, 3],
    dist [cameras, 14]) float64 from cfg.infer.calibration -- one calibration file for every camera (the reference's single
    K_dist) or a list of one per camera -- each rescaled to frame_size = (width, height) (formats.Calibration.scaled_to).
    A calibration whose coefficients are all zero describes a pinhole: with only such cameras the answer is None as well,
    so that "calibrated, no distortion" runs exactly what "no calibration" runs."""
    if not cfg_get(cfg, "infer.undistort", False):
        return None
    from . import formats
    paths = cfg_get(cfg, "infer.calibration", None)
    if paths is None:
        raise ValueError("cfg.infer.undistort is set but cfg.infer.calibration names no calibration file")
    paths = [paths] * cameras if isinstance(paths, (str, Path)) else [p for p in paths]
    if len(paths) != cameras:
        raise ValueError(f"cfg.infer.calibration: one path, or one per camera ({cameras}), got {len(paths)}")
    cals = [formats.load_calibration(p).scaled_to(*frame_size) for p in paths]
    K, dist = np.stack([c.K for c in cals]), np.stack([c.dist for c in cals])
    geometry.lens_coeffs(dist)   # refuses the tilt model before any frame is touched
    return (K, dist) if dist.any() else None


def undistort_detections(keypoints: np.ndarray, boxes: np.ndarray, K, dist, device):
    """One camera's detector output in source pixels under a lens: keypoints [..., 2] undistorted (geometry.undistort_points,
    P = K), boxes [..., 4] = (x1, y1, x2, y2) replaced by the bounding box of their four undistorted corners -> (keypoints,
    boxes, the largest finite resid_px, the number of finite points the inverse lost to NaN) with the inputs' dtypes."""
    with torch.cuda.device(device):
        kp_in = torch.from_numpy(np.ascontiguousarray(keypoints)).to(device)
        kp = geometry.undistort_points(kp_in, K, dist)
        b = torch.from_numpy(np.ascontiguousarray(boxes)).to(device)
        corners = torch.stack([b[..., [0, 1]], b[..., [2, 1]], b[..., [0, 3]], b[..., [2, 3]]], dim=-2)      # [..., 4, 2]
        c = geometry.undistort_points(corners, K, dist)
        nb = torch.cat([c.x.amin(dim=-2), c.x.amax(dim=-2)], dim=-1)
        resid = torch.cat([kp.resid_px.reshape(-1), c.resid_px.reshape(-1)])
        worst = float(torch.nan_to_num(resid, nan=0.0).max()) if resid.numel() else 0.0
        finite_in = torch.cat([torch.isfinite(kp_in).all(-1).reshape(-1), torch.isfinite(corners).all(-1).reshape(-1)])
        lost = int((finite_in & torch.isnan(resid)).sum())
        return kp.x.cpu().numpy().astype(keypoints.dtype), nb.cpu().numpy().astype(boxes.dtype), worst, lost


def predictions_to_glb_points(preds: dict, conf_thres=50.0, prediction_mode: str = "Predicted Pointmap", filter_by_frames="all",
                              mask_black_bg: bool = False, mask_white_bg: bool = False, mask_sky: bool = False):
    """The point cloud of the reference's predictions_to_glb (vggt/visual_util.py:39-236) from a prediction dict of DEVICE
    tensors, [S, ...] as the reference's or [B, S, ...] for B time steps at once -> geometry.SceneCloud (device).  The
    branch is the reference's (:89-101): "Pointmap" in prediction_mode takes world_points / world_points_conf, or without
    world_points falls back to world_points_from_depth / depth_conf; any other mode string ("All" included) takes the
    depth branch.  A missing confidence map is all ones.  conf_thres=None becomes 10 (:77-78).  filter_by_frames="k:..."
    keeps view k only (:82-87, :158-162), anything unparsable keeps all.  mask_sky needs a downloaded ONNX model and is not
    part of this build.  The camera cones of show_cam are not built: `scale` and `transform` are returned for a caller who
    adds them."""
    if not isinstance(preds, dict):
        raise ValueError("predictions must be a dictionary")
    if mask_sky:
        raise NotImplementedError("mask_sky needs the reference's downloaded sky-segmentation model (skyseg.onnx)")
    if conf_thres is None:
        conf_thres = 10.0
    selected = None
    if filter_by_frames != "all" and filter_by_frames != "All":
        try:
            selected = int(str(filter_by_frames).split(":")[0])
        except (ValueError, IndexError):
            pass
    if "Pointmap" in prediction_mode and "world_points" in preds:
        points, conf = preds["world_points"], preds.get("world_points_conf")
    else:
        points, conf = preds["world_points_from_depth"], preds.get("depth_conf")
    images, extrinsic = preds["images"], preds["extrinsic"]
    if points.dim() == 4:   # one time step, the reference's layout
        points, images, extrinsic = points[None], images[None], extrinsic[None]
        conf = None if conf is None else conf[None]
    if conf is None:
        conf = torch.ones_like(points[..., 0])
    if selected is not None:
        S = points.shape[1]
        if not -S <= selected < S:
            raise IndexError(f"filter_by_frames: view {selected} of {S}")
        k = selected % S
        points, conf, images, extrinsic = (x[:, k:k + 1] for x in (points, conf, images, extrinsic))
    return geometry.scene_point_cloud(points, conf, images, extrinsic, conf_thres=float(conf_thres), mask_black_bg=mask_black_bg,
                                      mask_white_bg=mask_white_bg)


class CameraHead:
    """Drop-in for vggt.vggt.infer.CameraHead (the reference-side VGGT wrapper)."""

    def __init__(self, cfg=None, out_dir: Optional[Path] = None, model: Optional[VGGT] = None, state_dict=None,
                 prec=PREC_BF16, head_prec=PREC_BF16X3):
        gpu = int(cfg_get(cfg, "infer.gpu", 0) or 0)   # configs/vggt.yaml infer.gpu
        if not torch.cuda.is_available():
            raise RuntimeError("VGGT needs a GPU.")   # infer.py:49-51
        self.device = f"cuda:{gpu}"
        torch.cuda.set_device(gpu)
        self.outdir = Path(out_dir) if out_dir is not None else None
        # the reference reads these two at the ROOT of the config (infer.py:56-57)
        self.conf_thres = cfg_get(cfg, "conf_thres", 50.0)
        self.prediction_mode = cfg_get(cfg, "prediction_mode", "All")
        if model is None and state_dict is None:
            ckpt = cfg_get(cfg, "infer.ckpt_path", None)     # offline stand-in for the URL of infer.py:62-66
            self.vggt = self.load_vggt_model(self.device, ckpt_path=ckpt, prec=prec, head_prec=head_prec)
        else:
            self.vggt = model if model is not None else self.load_vggt_model(self.device, state_dict=state_dict, prec=prec,
                                                                            head_prec=head_prec)

    @staticmethod
    def load_vggt_model(device="cuda", verbose=True, state_dict=None, ckpt_path=None, prec=PREC_BF16,
                        head_prec=PREC_BF16X3):
        """infer.py:59-69 fetches model.pt from a URL; offline, pass the same flat state_dict
        (or a local path to it)."""
        model = VGGT(prec=prec, head_prec=head_prec)
        if state_dict is None:
            if ckpt_path is None:
                raise RuntimeError("no network here: pass state_dict= or ckpt_path= (the reference's model.pt format)")
            state_dict = torch.load(ckpt_path, map_location="cpu", weights_only=True)
        model.load_state_dict(state_dict)
        return model.eval()

    @torch.no_grad()
    def run_vggt(self, images: List[torch.Tensor], to_numpy: bool = True):
        """infer.py:71-105.  Returns (out dict, H, W).  With to_numpy=False everything stays in HBM."""
        # RGB uint8 frames are resized on the GPU (bit-identical to the PIL path, preprocess.py);
        # anything else (RGBA, other dtypes) takes the reference's host path
        def _rgb8(im):
            return getattr(im, "dtype", None) in (torch.uint8, np.uint8) and getattr(im, "ndim", 0) == 3 and im.shape[2] == 3
        on_dev = all(_rgb8(im) for im in images)
        imgs = load_and_preprocess_images(images, device=self.device if on_dev else None).to(self.device)
        preds = self.vggt(imgs)
        H, W = imgs.shape[-2:]
        E, K = geometry.pose_encoding_to_extri_intri(preds["pose_enc"], (H, W))
        preds["extrinsic"], preds["intrinsic"] = E, K
        preds["world_points_from_depth"] = geometry.unproject_depth_map_to_point_map(
            preds["depth"][0], E[0], K[0])[None]
        if not to_numpy:
            return preds, H, W
        out = {k: (v.detach().cpu().numpy().squeeze(0) if isinstance(v, torch.Tensor) else v) for k, v in preds.items()}
        out["pose_enc_list"] = None
        return out, H, W

    extrinsic_to_RT = staticmethod(geometry.extrinsic_to_RT)
    scale_intrinsics = staticmethod(geometry.scale_intrinsics)

    def reconstruct_from_frames(self, frame_id: int, imgs: List[torch.Tensor]):
        """infer.py:157-215 -> (extrinsics [S,3,4], intrinsics rescaled to the source resolution
        (list of [3,3]), R [S,3,3], t [S,3], C [S,3], world_points_from_depth)."""
        return self.reconstruct_batch([frame_id], [imgs])[0]

    @torch.no_grad()
    def reconstruct_batch(self, frame_ids: Sequence[int], steps: Sequence[List[torch.Tensor]], write: Optional[Sequence[bool]] = None,
                          dense_to_host: bool = True, scene: bool = False):
        """`reconstruct_from_frames` for several independent time steps in ONE model call (B = len(steps),
        every step S frames of one source size): the steps of a clip are independent
        (vggt/multi_view_process.py:133), and batching them is what fills the chip.  Returns one
        reconstruct_from_frames tuple per step; per step `<outdir>/frame_XXXX/predictions.npz` holds the
        camera arrays of the reference's predictions.npz (vggt/save.py:52-56; the dense maps are returned,
        not written: the per-frame PNG / dense dumps are out of scope).  dense_to_host=False skips the host copy
        of the world points (26 MB at B = 4, S = 2, 518 x 518): that tuple slot is then None, and `last_world_points`
        still holds the device copy.  scene=True: one geometry.scene_point_cloud call builds the reference's filtered,
        coloured cloud of all B steps on the device (`predictions_to_glb_points` with this head's conf_thres and
        prediction_mode; the point head runs only when the mode asks for it), `last_scene` keeps the device result, and
        every written step also gets the reference's `scene_conf{conf_thres}_mode{mode}.glb` (vggt/save.py:59-61): only
        the kept rows cross to the host.  Everything else is what scene=False gives, bitwise."""
        B, S = len(steps), len(steps[0])
        H, W = steps[0][0].shape[:2]
        flat = [im for st in steps for im in st]
        if len(flat) != B * S:
            raise ValueError("every time step needs the same number of views")

        def _rgb8(im):
            return getattr(im, "dtype", None) in (torch.uint8, np.uint8) and getattr(im, "ndim", 0) == 3 and im.shape[2] == 3
        on_dev = all(_rgb8(im) for im in flat)
        imgs = load_and_preprocess_images(flat, device=self.device if on_dev else None).to(self.device)
        oh, ow = imgs.shape[-2:]
        want = {"camera", "depth"}
        if scene and "Pointmap" in self.prediction_mode:
            want = want | {"point"}
        preds = self.vggt(imgs.view(B, S, 3, oh, ow), want=want)
        E, K = geometry.pose_encoding_to_extri_intri(preds["pose_enc"], (oh, ow))
        wp = torch.stack([geometry.unproject_depth_map_to_point_map(preds["depth"][b], E[b], K[b]) for b in range(B)])
        self.last_world_points = wp   # the device copy of the returned maps [B, S, H, W, 3] (the ICP of process_multi_view_video)
        if scene:
            cloud = predictions_to_glb_points(dict(preds, world_points_from_depth=wp, images=imgs.view(B, S, 3, oh, ow), extrinsic=E),
                                              self.conf_thres, self.prediction_mode)
            self.last_scene = cloud
            kept = torch.clamp(cloud.count, max=cloud.xyz.shape[1]).cpu().tolist()
        En, Kn, pen = E.cpu().numpy(), K.cpu().numpy(), preds["pose_enc"].cpu().numpy()
        wpn = wp.cpu().numpy() if dense_to_host else [None] * B
        out = []
        for b in range(B):
            R, t, C = self.extrinsic_to_RT(En[b])
            K_resized = [self.scale_intrinsics(Kn[b, i], orig_size=(oh, ow), new_size=(H, W)) for i in range(S)]
            if self.outdir is not None and (write is None or write[b]):
                d = self.outdir / f"frame_{int(frame_ids[b]):04d}"
                d.mkdir(parents=True, exist_ok=True)
                np.savez(d / "predictions.npz", extrinsic=En[b], intrinsic=Kn[b], pose_enc=pen[b])
                if scene:
                    from . import formats
                    name = f"scene_conf{self.conf_thres}_mode{self.prediction_mode.replace(' ', '_')}.glb"
                    formats.write_glb_points(d / name, cloud.xyz[b, :kept[b]].cpu().numpy(), cloud.rgb[b, :kept[b]].cpu().numpy())
            out.append((En[b], K_resized, R, t, C, wpn[b]))
        return out


def save_camera_info(out_pt_path: Path, all_frame_camera_intrinsics, all_frame_R, all_frame_t, all_frame_C,
                     all_frame_x3d=None, extra: Optional[dict] = None):
    """vggt/save.py:84-110 (NPZ with camera_intrinsics [N,C,3,3], R [N,C,3,3], t [N,C,3], C [N,C,3]);
    accepts the all_frame_x3d the reference's caller passes (multi_view_process.py:312-319)."""
    data = {"camera_intrinsics": np.stack(all_frame_camera_intrinsics, axis=0), "R": np.stack(all_frame_R, axis=0),
            "t": np.stack(all_frame_t, axis=0), "C": np.stack(all_frame_C, axis=0)}
    if all_frame_x3d is not None:
        data["x3d"] = np.stack(all_frame_x3d, axis=0)
    if extra:
        data.update(extra)      # build-side additions (e.g. icp_refined, x3d_smoothed); the reference's keys are untouched
    np.savez_compressed(Path(out_pt_path).with_suffix(".npz"), **data)


_SIDE_STREAMS: Dict = {}


def _side_streams(dev, n):
    """n long-lived side streams of a device (the model keeps one workspace per stream it has run on)"""
    pool = _SIDE_STREAMS.setdefault(torch.device(dev), [])
    while len(pool) < n:
        pool.append(torch.cuda.Stream(dev))
    return pool[:n]


_H36M_KEYS = ("joints3d", "joints3d_smoothed", "joints3d_clean", "joints3d_clean_smoothed", "joints3d_robust", "joints3d_robust_ok",
              "joints3d_robust_smoothed")


def _with_h36m(out, skeleton):
    """process_multi_view_clip(skeleton="h36m"): the COCO-17 joint keys that are present, converted under <key>_h36m"""
    if skeleton is None:
        return out
    for key in _H36M_KEYS:
        if key in out:
            x = out[key]
            out[key + "_h36m"] = geometry.convert_skeleton(x if x.is_cuda else x.numpy(), "coco_to_h36m")
    return out


@torch.no_grad()
def process_multi_view_clip(model: VGGT, frames: torch.Tensor, keypoints: torch.Tensor, steps_per_call: int = 4,
                            want_dense: bool = False, streams: int = 1, smooth: bool = False, boxes: Optional[torch.Tensor] = None,
                            scores: Optional[torch.Tensor] = None, source_size=None, triage: bool = False,
                            conf_thr: float = 0.3, err_thresh_px: float = 2.0, robust: bool = False,
                            inlier_px: Optional[float] = None, min_inliers: int = 2, refine_iters: int = 5,
                            weighted: bool = False, device_smooth: bool = False,
                            skeleton: Optional[str] = None) -> Dict[str, torch.Tensor]:
    """The hot loop of process_multi_view_video (vggt/multi_view_process.py:133-309) for a clip
    already in memory: frames [T, S, 3, H, W] in [0,1] (device), keypoints [T, S, J, 2] in the
    pixels of the H x W frames.  Per time step: one S-view VGGT call -> cameras -> DLT
    triangulation of the J joints over the S views.

    Under torch.distributed the T time steps are split in contiguous blocks across ranks and the
    [T, J, 3] joints (+ cameras) are re-assembled on every rank with ONE all-gather of packed per-step
    records (parallel.all_gather_packed).  smooth=True chains BASELINE config 4's last stage on the gathered
    joints: `fuse.temporal_smooth_ema` (fuse/fuse.py:329-412) -> "joints3d_smoothed" [T, J, 3] float64 (host).
    device_smooth=True (with smooth=True) computes the smoothed keys with geometry.smooth_ema / geometry.smooth_savgol
    instead and returns them as device float64 tensors: the joints are not read back.  Off (the default), the function
    is what it was.

    streams > 1: the calls of this rank (chunks of steps_per_call time steps, independent of each
    other) are issued from that many host threads on as many HIP streams, so the HBM-bound phases of
    one call (GEMM store bursts, LayerNorm, upsamples) overlap the MFMA-bound phases of another:
    measured +5.5 % frames/s at 2 x 4 time steps in flight on one MI355X (tools/two_streams.py).

    boxes [T, S, 4] (device; detector boxes x1, y1, x2, y2 in the pixels of a `source_size` = (height, width) image,
    default the frames' own H x W): the joints come out in the reference's person-centred frame
    (multi_view_process.py:176-217).  The call then also asks the model for depth, unprojects it, takes the S person
    origins of the step (geometry.person_origin), moves the world origin onto their mean and, at S = 2, turns view 1
    (geometry.recenter_cameras); the dict gains "origin" [T, 3] float64 and the cameras the joints were triangulated
    with, "R" [T, S, 3, 3] and "t" [T, S, 3].  triage=True: geometry.triangulate_triage replaces the plain DLT (scores
    [T, S, J], optional, are the detector's keypoint scores) and the dict gains "joints3d_clean", "reproj_err" [T, S, J],
    "keep" [T, J] bool, "view_stats" [T, S, 4], "triage_report" [T, 5]; with smooth=True also
    "joints3d_clean_smoothed" (fuse.smooth_skeleton).  All of it runs on the device between the model call and the
    gather, without a host copy or a host wait, and travels in the same single packed all-gather.  Without these
    arguments the function does what it did before them.

    robust=True: geometry.triangulate_robust runs as well, on the same cameras (the recentred ones with `boxes`), keypoints
    and scores (conf_thr as for triage; inlier_px defaults to err_thresh_px; min_inliers, refine_iters, weighted as
    there), and the dict gains "joints3d_robust", "joints3d_robust_ok", "robust_err" [T, S, J], "inlier_views" [T, J]
    uint8, "robust_rms_px" [T, J], "robust_ok" [T, J] bool, "view_inlier_ratio" [T, S], "robust_report" [T, 4]; with
    smooth=True also "joints3d_robust_smoothed" = fuse.smooth_skeleton(joints3d_robust_ok).  "joints3d" and the triage
    outputs stay what they are: robust and triage are independent and may both be on.  2 <= S <= 8, J <= 32.

    skeleton="h36m" (default None: nothing changes): the keypoints are COCO-17 (J = 17, anything else is a ValueError before
    the model is called) and the dict gains "joints3d_h36m" [T, 17, 3], the H36M-17 form of "joints3d" (geometry.
    convert_skeleton, "coco_to_h36m"), float64 on the device, which geometry.kinematics (angle.H36M_17), geometry.fuse_h36m
    and geometry.pose_errors take; the smoothed, clean and robust joint keys that are present are converted the same way
    under "<key>_h36m".  Every other key is what it is without the argument."""
    T, S = frames.shape[:2]
    if skeleton is not None:
        if skeleton != "h36m":
            raise ValueError(f"process_multi_view_clip: skeleton must be None or 'h36m', got {skeleton!r}")
        if keypoints.dim() != 4 or keypoints.shape[2] != 17:
            raise ValueError(f"process_multi_view_clip: skeleton='h36m' converts COCO-17 joints, keypoints are "
                             f"{list(keypoints.shape)}")
    H, W = frames.shape[-2:]
    lo, hi, T_pad = parallel.shard_range(T)
    want = {"camera", "depth", "point"} if want_dense else {"camera"}
    if boxes is not None:
        want = want | {"depth"}
        if not boxes.is_cuda or tuple(boxes.shape) != (T, S, 4):
            raise ValueError(f"process_multi_view_clip: boxes must be a device tensor {[T, S, 4]}, got {list(boxes.shape)} "
                             f"on {boxes.device}")
        src = (H, W) if source_size is None else (int(source_size[0]), int(source_size[1]))
    if scores is not None and not (triage or robust):
        raise ValueError("process_multi_view_clip: scores are only read by triage=True or robust=True")
    if robust:   # what skimi_triangulate_robust would refuse, refused before the model is called
        inlier_px = float(err_thresh_px if inlier_px is None else inlier_px)
        min_inliers, refine_iters = int(min_inliers), int(refine_iters)
        Jk = keypoints.shape[2] if keypoints.dim() == 4 else -1
        if not 2 <= S <= geometry.ROBUST_MAX_VIEWS or not 1 <= Jk <= geometry.ROBUST_MAX_JOINTS:
            raise ValueError(f"process_multi_view_clip: robust=True needs 2..8 views and 1..32 joints, got frames "
                             f"{list(frames.shape)}, keypoints {list(keypoints.shape)}")
        if not 2 <= min_inliers <= S:
            raise ValueError(f"process_multi_view_clip: min_inliers must be in 2..{S} (the views), got {min_inliers}")
        if not 0 <= refine_iters <= geometry.ROBUST_MAX_REFINE_ITERS:
            raise ValueError(f"process_multi_view_clip: refine_iters must be in 0..{geometry.ROBUST_MAX_REFINE_ITERS}, got "
                             f"{refine_iters}")
        if not inlier_px >= 0:
            raise ValueError(f"process_multi_view_clip: inlier_px must be >= 0, got {inlier_px}")
    if boxes is not None or triage or robust:   # these reach the kernels as raw pointers: device tensors of the clip's shape only
        J = keypoints.shape[2] if keypoints.dim() == 4 else -1
        if not keypoints.is_cuda or tuple(keypoints.shape) != (T, S, J, 2):
            raise ValueError(f"process_multi_view_clip: keypoints must be a device tensor [{T}, {S}, J, 2], got "
                             f"{list(keypoints.shape)} on {keypoints.device}")
        if scores is not None and (not scores.is_cuda or tuple(scores.shape) != (T, S, J)):
            raise ValueError(f"process_multi_view_clip: scores must be a device tensor {[T, S, J]}, got "
                             f"{list(scores.shape)} on {scores.device}")
    starts = list(range(lo, hi, steps_per_call))

    n_par = max(1, min(int(streams), len(starts) - 1))

    def one_call(a):
        b = min(a + steps_per_call, hi)
        idx = [min(i, T - 1) for i in range(a, b)]          # padded steps repeat the last one
        n = len(idx)
        out = model(frames[idx], want=want)
        E, K = geometry.pose_encoding_to_extri_intri(out["pose_enc"], (H, W))
        R, t = E[..., :3, :3].contiguous(), E[..., :3, 3].contiguous()
        if boxes is None and not triage and not robust:
            return geometry.triangulate_joints(K, R, t, keypoints[idx])[:n], E[:n], K[:n]
        # from here to the gather nothing crosses to the host and the host waits for nothing: the steps' slices of
        # boxes / keypoints / scores are taken on the device (a list index would upload an index tensor)
        # steps a .. b-1, those at or beyond T repeating step T-1 (a chunk of a padded shard may lie wholly beyond T)
        def steps_of(x):
            if b <= T:
                return x[a:b]
            return torch.cat([x[min(a, T):T], x[T - 1:T].expand(b - max(a, T), *x.shape[1:])])

        extra = []
        if boxes is not None:
            depth = out["depth"]
            oh, ow = depth.shape[2:4]
            wp = geometry.unproject_depth_map_to_point_map(depth.reshape(n * S, oh, ow, -1), E.reshape(n * S, 3, 4),
                                                           K.reshape(n * S, 3, 3))
            stats = geometry.person_stats(wp, steps_of(boxes).reshape(n * S, 4).contiguous().to(torch.float32), src)
            origin, R, t = geometry.recenter_cameras(stats.view(n, S, 8), E)
            extra = [origin, R, t]
        if not triage and not robust:
            return (geometry.triangulate_joints(K, R, t, steps_of(keypoints)), E, K, *extra)
        kp = steps_of(keypoints).contiguous().to(torch.float32)
        conf = None if scores is None else steps_of(scores).contiguous().to(torch.float32)
        Kc = K.contiguous()
        if triage:
            X, Xc, err, _depth, keep, vs, rep = geometry.triage_launch(Kc, R, t, kp, conf, conf_thr, err_thresh_px)
            extra += [Xc, err, keep, vs, rep]
        else:
            X = geometry.triangulate_joints(K, R, t, kp)
        if robust:
            extra += geometry.robust_launch(Kc, R, t, kp, conf, conf_thr, inlier_px, min_inliers, refine_iters, weighted)
        return (X, E, K, *extra)

    results = [None] * len(starts)
    if n_par <= 1:
        for i, a in enumerate(starts):
            results[i] = one_call(a)
    else:
        import threading

        dev = frames.device
        main = torch.cuda.current_stream(dev)
        results[0] = one_call(starts[0])    # sizes this stream's workspace before the side streams start
        side = _side_streams(dev, n_par)
        errors = []

        def worker(k):
            try:
                with torch.cuda.device(dev), torch.cuda.stream(side[k]):
                    for i in range(1 + k, len(starts), n_par):
                        results[i] = one_call(starts[i])
            except BaseException as e:   # re-raised on the calling thread
                errors.append(e)

        for s in side:
            s.wait_stream(main)
        threads = [threading.Thread(target=worker, args=(k,)) for k in range(n_par)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        for s in side:
            main.wait_stream(s)
        if errors:
            raise errors[0]
        for r in results:   # the side streams' results are read on the caller's stream from here on
            for x in r:
                x.record_stream(main)
    # the path's ONE collective: joints + cameras (+ origin, triage verdicts, robust joints) of this rank's steps as one packed record
    # per step
    names = ["joints3d", "extrinsic", "intrinsic"] + (["origin", "R", "t"] if boxes is not None else []) + (
        ["joints3d_clean", "reproj_err", "keep", "view_stats", "triage_report"] if triage else []) + (
        ["joints3d_robust", "robust_err", "inlier_views", "robust_rms_px", "robust_ok", "joints3d_robust_ok", "view_inlier_ratio",
         "robust_report"] if robust else [])
    parts = parallel.all_gather_packed([torch.cat([r[k] for r in results]) for k in range(len(names))], T)
    out = dict(zip(names, parts))
    joints = out["joints3d"]
    if triage:
        out["keep"] = out["keep"].bool()
    if robust:
        out["robust_ok"] = out["robust_ok"].bool()
    if smooth:
        # BASELINE config 4: after the gather, fuse/'s temporal smoothing over the whole clip (sequential in t,
        # O(T J) on the host as in the reference: fuse/fuse.py:329-412); every rank holds the same result
        from . import fuse
        if device_smooth:   # the same three keys as device float64 tensors: the joints never leave the device
            out["joints3d_smoothed"] = geometry.smooth_ema(joints).X
            if triage:
                out["joints3d_clean_smoothed"] = geometry.smooth_savgol(out["joints3d_clean"]).X
            if robust:
                out["joints3d_robust_smoothed"] = geometry.smooth_savgol(out["joints3d_robust_ok"]).X
            return _with_h36m(out, skeleton)
        out["joints3d_smoothed"] = torch.from_numpy(fuse.temporal_smooth_ema(joints.cpu().numpy().astype(np.float64)))
        if triage:   # the reference's post_triage_sequence(smooth=True): Savitzky-Golay over the kept joints
            out["joints3d_clean_smoothed"] = torch.from_numpy(
                fuse.smooth_skeleton(out["joints3d_clean"].cpu().numpy().astype(np.float64)))
        if robust:   # the same filter over the joints the consensus accepted
            out["joints3d_robust_smoothed"] = torch.from_numpy(
                fuse.smooth_skeleton(out["joints3d_robust_ok"].cpu().numpy().astype(np.float64)))
    return _with_h36m(out, skeleton)


@torch.no_grad()
def process_single_view_clip(model: VGGT, frames: torch.Tensor, every: int = 30):
    """vggt/single_view_process.py:130-170: every `every`-th frame of ONE camera forms a single
    S = ceil(T/every) call; returns the cameras of those frames.  frames [T, 3, H, W] (device)."""
    sel = frames[::every]
    H, W = sel.shape[-2:]
    out = model(sel, want={"camera"})
    E, K = geometry.pose_encoding_to_extri_intri(out["pose_enc"], (H, W))
    return {"extrinsic": E[0], "intrinsic": K[0], "pose_enc": out["pose_enc"][0]}


def render_scene_views(cloud, extrinsic, intrinsic, joints=None, links=None, scene: int = 0, size=(518, 518), image_size=None, orbit=None,
                       point_size: int = 1, aligned: bool = True, cameras: bool = True, background=(255, 255, 255), want_index: bool = False):
    """The scene of a VGGT step as pictures, fed directly from CameraHead.last_scene: cloud geometry.SceneCloud (its count stays
    on the device: the renderer reads it), extrinsic [S, 3, 4], intrinsic [S, 3, 3] the step's cameras (device), joints [J, 3]
    world joints with `links` or None -> geometry.SceneView with frames uint8 [F, H, W, 3] (RGB, as the cloud's colours).
    orbit=None: F = S, the scene seen from its own cameras (intrinsic is for images of image_size = (H, W), default `size`).
    orbit=(frames, elev_deg): an orbit of that many frames about the z axis through the middle of the cloud's 5 .. 95 % box,
    at 1.2 scene scales.  cameras=True adds every camera's axes and frustum.  aligned=True: the cloud was written with
    scene_point_cloud(align=True), so cameras and joints are moved by cloud.transform to the cloud's frame.  Everything is
    computed on the device; nothing is read back."""
    dev = cloud.xyz.device
    E = torch.as_tensor(extrinsic).to(dev, torch.float64)
    K = torch.as_tensor(intrinsic).to(dev, torch.float64)
    if E.dim() != 3 or E.shape[-2:] != (3, 4) or tuple(K.shape) != (E.shape[0], 3, 3):
        raise ValueError(f"render_scene_views: need extrinsic [S, 3, 4] and intrinsic [S, 3, 3], got {list(E.shape)}, {list(K.shape)}")
    H, W = int(size[0]), int(size[1])
    b = int(scene)
    T = cloud.transform[b]
    scale = cloud.scale[b]
    mid = 0.5 * (cloud.lower[b] + cloud.upper[b])                       # in the raw world frame
    j = None if joints is None else torch.as_tensor(joints).to(dev, torch.float64)
    if aligned:   # x' = T x: a camera [R|t] of the raw frame is [R|t] T^-1 in the cloud's
        # inv_ex: the inverse without linalg.inv's check of the status on the host (a singular transform gives non-finite
        # views, which draw nothing)
        bottom = geometry.host_const([[0.0, 0.0, 0.0, 1.0]], torch.float64, dev).expand(E.shape[0], 1, 4)
        E = (torch.cat([E, bottom], dim=1) @ torch.linalg.inv_ex(T).inverse)[:, :3]
        mid = T[:3, :3] @ mid + T[:3, 3]
        j = None if j is None else j @ T[:3, :3].T + T[:3, 3]
    if orbit is None:
        if image_size is not None:
            sx, sy = W / float(image_size[1]), H / float(image_size[0])
            K = K * geometry.host_const([[sx, 1.0, sx], [1.0, sy, sy], [1.0, 1.0, 1.0]], torch.float64, dev)
        views = geometry.views_from_cameras(E, K, near=0.01 * scale, far=100.0 * scale)
    else:
        n, elev = int(orbit[0]), float(orbit[1])
        az = torch.arange(n, dtype=torch.float64, device=dev) * (360.0 / max(n, 1))
        views = geometry.orbit_view(mid, 1.2 * scale, elev, az, 0.8 * W, 0.8 * W, W / 2.0, H / 2.0, 0.01 * scale, 4.0 * scale)
    lists = []
    if cameras:
        lists.append(geometry.camera_prims(E, K, views, 0.05 * scale, 0.05 * scale))
    if j is not None:
        lists.append(geometry.skeleton_prims(j, links or [], views))
    prims = geometry.cat_prims(*lists) if lists else None
    return geometry.render_scene(views, cloud.xyz[b:b + 1], cloud.rgb[b:b + 1], count=cloud.count[b:b + 1].clamp(max=cloud.xyz.shape[1]),
                                 point_size=point_size, prims=prims, size=(H, W), background=background, want_index=want_index)
