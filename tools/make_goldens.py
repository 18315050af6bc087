#!/usr/bin/env python
"""Generate tests/golden/*.npz by running the REFERENCE's own model classes
(imported from /root/reference, never copied) on this build's deterministic synthetic
weights and inputs.  Runs only in the build container (the GPU box has no reference).

Fixtures hold data only: seeds/config, inputs, and the reference's outputs.  Weights are
rebuilt from (spec, seed) by skiing_analysis_pytorch_amd.weights on whichever machine runs
the tests, so they are not stored.

    PYTHONPATH=/root/reference PYTHONDONTWRITEBYTECODE=1 python tools/make_goldens.py [vp3d|vp3d_dense|vggt_tiny|...]
"""
from __future__ import annotations

import os
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
REF = os.environ.get("SKIMI_REFERENCE", "/root/reference")
sys.path.insert(0, REF)
sys.dont_write_bytecode = True

GOLD = ROOT / "tests" / "golden"
GOLD.mkdir(parents=True, exist_ok=True)

from skiing_analysis_pytorch_amd import weights as W  # noqa: E402

torch.set_grad_enabled(False)
torch.manual_seed(0)


def gen_vp3d():
    from VideoPose3D.common.camera import normalize_screen_coordinates
    from VideoPose3D.common.generators import UnchunkedGenerator
    from VideoPose3D.common.model import TemporalModel

    kps_left, kps_right = [1, 3, 5, 7, 9, 11, 13, 15], [2, 4, 6, 8, 10, 12, 14, 16]
    joints_left, joints_right = [4, 5, 6, 11, 12, 13], [1, 2, 3, 14, 15, 16]
    W_, H_ = 1920, 1080
    for name, fw, causal, frames in (
        ("rf27", [3, 3, 3], False, 243),
        ("rf27_causal", [3, 3, 3], True, 60),
        ("rf243", [3, 3, 3, 3, 3], False, 243),
        ("rf81_w5", [3, 3, 3, 3], False, 40),
    ):
        sd = W.make_vp3d_state_dict(seed=0, filter_widths=fw)
        m = TemporalModel(17, 2, 17, filter_widths=fw, causal=causal, channels=1024).eval()
        m.load_state_dict(sd, strict=True)
        kp = W.make_keypoints_2d(frames=frames, seed=1).numpy()
        kps_n = normalize_screen_coordinates(kp.astype(np.float64), w=W_, h=H_)
        rf = m.receptive_field()
        pad = (rf - 1) // 2
        shift = pad if causal else 0
        out = {}
        for aug in (False, True):
            gen = UnchunkedGenerator(None, None, [kps_n], pad=pad, causal_shift=shift, augment=aug,
                                     kps_left=kps_left, kps_right=kps_right, joints_left=joints_left,
                                     joints_right=joints_right)
            for _, _, batch_2d in gen.next_epoch():
                x = torch.from_numpy(batch_2d.astype("float32"))
                pred = m(x)
                out[f"batch2d_aug{int(aug)}"] = batch_2d.astype(np.float32)
                out[f"raw_aug{int(aug)}"] = pred.numpy().copy()
                if aug:  # VideoPose3D/run.py:979-986
                    pred[1, :, :, 0] *= -1
                    pred[1, :, joints_left + joints_right] = pred[1, :, joints_right + joints_left]
                    pred = torch.mean(pred, dim=0, keepdim=True)
                out[f"pred_aug{int(aug)}"] = pred.squeeze(0).numpy()
        np.savez_compressed(GOLD / f"vp3d_{name}.npz", filter_widths=np.array(fw), causal=np.array(causal),
                            seed=np.array(0), kp_seed=np.array(1), frames=np.array(frames), w=np.array(W_),
                            h=np.array(H_), keypoints_px=kp, receptive_field=np.array(rf), **out)
        print("wrote", f"vp3d_{name}.npz", {k: v.shape for k, v in out.items()})


def gen_vp3d_dense():
    """TemporalModel(dense=True) (VideoPose3D/common/model.py:113-116): the same fields as gen_vp3d, plus the shapes
    of the conv weights (data only; the weights themselves are rebuilt from the seed)."""
    from VideoPose3D.common.camera import normalize_screen_coordinates
    from VideoPose3D.common.generators import UnchunkedGenerator
    from VideoPose3D.common.model import TemporalModel

    kps_left, kps_right = [1, 3, 5, 7, 9, 11, 13, 15], [2, 4, 6, 8, 10, 12, 14, 16]
    joints_left, joints_right = [4, 5, 6, 11, 12, 13], [1, 2, 3, 14, 15, 16]
    W_, H_ = 1920, 1080
    for name, fw, causal, frames in (
        ("rf27_dense", [3, 3, 3], False, 243),
        ("rf27_dense_causal", [3, 3, 3], True, 60),
        ("rf243_dense", [3, 3, 3, 3, 3], False, 243),
        ("w535_dense", [3, 5, 3], False, 40),     # 13 and 31 taps
    ):
        sd = W.make_vp3d_state_dict(seed=0, filter_widths=fw, dense=True)
        m = TemporalModel(17, 2, 17, filter_widths=fw, causal=causal, channels=1024, dense=True).eval()
        m.load_state_dict(sd, strict=True)
        conv_keys = [k for k, v in m.state_dict().items() if v.dim() == 3]
        conv_shapes = np.array([list(m.state_dict()[k].shape) for k in conv_keys], dtype=np.int64)
        kp = W.make_keypoints_2d(frames=frames, seed=1).numpy()
        kps_n = normalize_screen_coordinates(kp.astype(np.float64), w=W_, h=H_)
        rf = m.receptive_field()
        pad = (rf - 1) // 2
        shift = pad if causal else 0
        out = {}
        for aug in (False, True):
            gen = UnchunkedGenerator(None, None, [kps_n], pad=pad, causal_shift=shift, augment=aug,
                                     kps_left=kps_left, kps_right=kps_right, joints_left=joints_left,
                                     joints_right=joints_right)
            for _, _, batch_2d in gen.next_epoch():
                x = torch.from_numpy(batch_2d.astype("float32"))
                pred = m(x)
                out[f"batch2d_aug{int(aug)}"] = batch_2d.astype(np.float32)
                out[f"raw_aug{int(aug)}"] = pred.numpy().copy()
                if aug:  # VideoPose3D/run.py:979-986
                    pred[1, :, :, 0] *= -1
                    pred[1, :, joints_left + joints_right] = pred[1, :, joints_right + joints_left]
                    pred = torch.mean(pred, dim=0, keepdim=True)
                out[f"pred_aug{int(aug)}"] = pred.squeeze(0).numpy()
        path = GOLD / f"vp3d_{name}.npz"
        np.savez_compressed(path, filter_widths=np.array(fw), causal=np.array(causal), dense=np.array(True),
                            seed=np.array(0), kp_seed=np.array(1), frames=np.array(frames), w=np.array(W_),
                            h=np.array(H_), keypoints_px=kp, receptive_field=np.array(rf),
                            conv_weight_keys=np.array(conv_keys), conv_weight_shapes=conv_shapes, **out)
        print("wrote", path.name, path.stat().st_size, "bytes", dict(zip(conv_keys, conv_shapes.tolist())))


TINY_CONFIGS = {
    # conv patch embed, everything on: exercises aggregator, camera, both DPT heads, track head
    "tiny_conv": dict(S=3, H=140, W=140, queries=5, cfg=dict(
        img_size=140, embed_dim=128, depth=4, num_heads=2, patch_embed="conv", cam_trunk_depth=2, cam_heads=2,
        dpt_features=128, dpt_out_channels=(64, 128, 256, 256), dpt_layers=(0, 1, 2, 3), track_features=64,
        track_hidden=128, track_corr_levels=3, track_corr_radius=3, track_iters=3, track_depth=2,
        track_heads=8, track_virtual=16)),
    # DINOv2 ViT-S/14-reg patch embed (12 blocks, LayerNorm eps 1e-6, LayerScale), no track head
    "tiny_dino_rect": dict(S=2, H=42, W=70, queries=0, cfg=dict(   # non-square: resized pos_embed
        img_size=70, embed_dim=384, depth=2, num_heads=6, patch_embed="dinov2_vits14_reg", dino_depth=12,
        dino_heads=6, cam_trunk_depth=1, cam_heads=6, dpt_features=64, dpt_out_channels=(64, 64, 128, 128),
        dpt_layers=(0, 0, 1, 1), enable_track=False)),
    "tiny_dino": dict(S=2, H=70, W=70, queries=0, cfg=dict(
        img_size=70, embed_dim=384, depth=2, num_heads=6, patch_embed="dinov2_vits14_reg", dino_depth=12,
        dino_heads=6, cam_trunk_depth=1, cam_heads=6, dpt_features=64, dpt_out_channels=(64, 64, 128, 128),
        dpt_layers=(0, 0, 1, 1), enable_track=False)),
}


def build_reference_vggt(cfg: "W.VGGTConfig"):
    """The reference VGGT module with non-default sizes: VGGT.__init__ hard-codes VGGT-1B, so the
    sub-modules are built with the reference's own classes and attached under the same attribute
    names; forward() is the reference's VGGT.forward unchanged."""
    import torch.nn as nn
    from vggt.vggt.heads.camera_head import CameraHead
    from vggt.vggt.heads.dpt_head import DPTHead
    from vggt.vggt.heads.track_head import TrackHead
    from vggt.vggt.models.aggregator import Aggregator
    from vggt.vggt.models.vggt import VGGT

    m = VGGT.__new__(VGGT)
    nn.Module.__init__(m)
    m.aggregator = Aggregator(img_size=cfg.img_size, patch_size=cfg.patch_size, embed_dim=cfg.embed_dim,
                              depth=cfg.depth, num_heads=cfg.num_heads, patch_embed=cfg.patch_embed)
    D = 2 * cfg.embed_dim
    m.camera_head = CameraHead(dim_in=D, trunk_depth=cfg.cam_trunk_depth, num_heads=cfg.cam_heads) if cfg.enable_camera else None
    dk = dict(dim_in=D, features=cfg.dpt_features, out_channels=list(cfg.dpt_out_channels),
              intermediate_layer_idx=list(cfg.dpt_layers))
    m.point_head = DPTHead(output_dim=4, activation="inv_log", conf_activation="expp1", **dk) if cfg.enable_point else None
    m.depth_head = DPTHead(output_dim=2, activation="exp", conf_activation="expp1", **dk) if cfg.enable_depth else None
    if cfg.enable_track:
        th = TrackHead(dim_in=D, patch_size=cfg.patch_size, features=cfg.track_features, iters=cfg.track_iters,
                       corr_levels=cfg.track_corr_levels, corr_radius=cfg.track_corr_radius,
                       hidden_size=cfg.track_hidden)
        # TrackHead builds its DPT with default out_channels/layers and its tracker with depth 6 /
        # 64 virtual tracks; rebuild those two with the reference classes for the tiny sizes
        from vggt.vggt.heads.track_modules.base_track_predictor import BaseTrackerPredictor
        from vggt.vggt.heads.track_modules.blocks import EfficientUpdateFormer
        th.feature_extractor = DPTHead(dim_in=D, patch_size=cfg.patch_size, features=cfg.track_features,
                                       out_channels=list(cfg.dpt_out_channels),
                                       intermediate_layer_idx=list(cfg.dpt_layers), feature_only=True,
                                       down_ratio=2, pos_embed=False)
        th.tracker = BaseTrackerPredictor(latent_dim=cfg.track_features, predict_conf=True, stride=2,
                                          corr_levels=cfg.track_corr_levels, corr_radius=cfg.track_corr_radius,
                                          hidden_size=cfg.track_hidden, depth=cfg.track_depth)
        th.tracker.updateformer = EfficientUpdateFormer(
            space_depth=cfg.track_depth, time_depth=cfg.track_depth, input_dim=3 * cfg.track_features + 4,
            hidden_size=cfg.track_hidden, num_heads=cfg.track_heads, output_dim=cfg.track_features + 2,
            mlp_ratio=4.0, add_space_attn=True, num_virtual_tracks=cfg.track_virtual)
        m.track_head = th
    else:
        m.track_head = None
    return m.eval()


def run_reference_vggt(name, cfgd, S, H, W_, nq, seed=0):
    cfg = W.VGGTConfig(**cfgd)
    sd = W.make_vggt_state_dict(cfg, seed=seed)
    m = build_reference_vggt(cfg)
    missing, unexpected = m.load_state_dict(sd, strict=True)
    images = W.make_images(S, H, W_, seed=seed + 1)
    q = None
    if nq:
        g = torch.Generator().manual_seed(seed + 2)
        q = torch.rand((nq, 2), generator=g) * torch.tensor([W_ - 20.0, H - 20.0]) + 10.0
    captured = {}
    hook = m.aggregator.register_forward_hook(lambda mod, i, o: captured.__setitem__("tokens", o[0]))
    preds = m(images, query_points=q)
    hook.remove()
    out = {"images_seed": np.array(seed + 1), "S": np.array(S), "H": np.array(H), "W": np.array(W_)}
    if q is not None:
        out["query_points"] = q.numpy()
    for k, v in preds.items():
        if k == "images":
            continue
        if k == "pose_enc_list":
            out[k] = torch.stack(v).numpy()
        else:
            out[k] = v.numpy()
    toks = captured["tokens"]
    out["tokens_last"] = toks[-1].numpy()
    out["tokens_first"] = toks[0].numpy()
    return cfg, out


def gen_vggt_tiny():
    import json

    for name, spec in TINY_CONFIGS.items():
        cfg, out = run_reference_vggt(name, spec["cfg"], spec["S"], spec["H"], spec["W"], spec["queries"])
        np.savez_compressed(GOLD / f"vggt_{name}.npz", cfg_json=np.array(json.dumps(spec["cfg"])), seed=np.array(0), **out)
        print("wrote", f"vggt_{name}.npz", {k: getattr(v, "shape", None) for k, v in out.items()})


GENERATORS = {"vp3d": gen_vp3d, "vp3d_dense": gen_vp3d_dense, "vggt_tiny": gen_vggt_tiny}



def gen_fuse():
    """fuse/fuse.py (pure NumPy): fuse_frame_3d + temporal_smooth_ema on a synthetic MHR-70-id
    sequence with missing joints (NaN) on either side."""
    from fuse.fuse import fuse_frame_3d, temporal_smooth_ema

    rng = np.random.default_rng(0)
    ids = [1, 2, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 41, 62, 69, 20, 33]
    T, J = 40, len(ids)
    base = rng.normal(size=(1, J, 3))
    L = base + np.cumsum(rng.normal(scale=0.03, size=(T, J, 3)), axis=0)
    R = L + rng.normal(scale=0.02, size=(T, J, 3))
    miss_l = rng.random((T, J)) < 0.08
    miss_r = rng.random((T, J)) < 0.08
    ql, qr = rng.normal(size=(T, J)), rng.normal(size=(T, J))
    fused = np.full((T, J, 3), np.nan)
    seq = []
    for t in range(T):
        dl = {jid: L[t, j] for j, jid in enumerate(ids) if not miss_l[t, j]}
        dr = {jid: R[t, j] for j, jid in enumerate(ids) if not miss_r[t, j]}
        if not dl:
            dl = {ids[0]: L[t, 0]}
        if not dr:
            dr = {ids[0]: R[t, 0]}
        f = fuse_frame_3d(dl, dr, ql[t], qr[t], ids)
        seq.append(f)
        for j, jid in enumerate(ids):
            if jid in f:
                fused[t, j] = f[jid]
    out = {}
    for name, kw in (("adaptive", dict()), ("plain", dict(adaptive=False, alpha=0.6))):
        sm = temporal_smooth_ema(seq, ids, **kw)
        Y = np.full((T, J, 3), np.nan)
        for t in range(T):
            for j, jid in enumerate(ids):
                if jid in sm[t]:
                    Y[t, j] = sm[t][jid]
        out["smooth_" + name] = Y
    np.savez_compressed(GOLD / "fuse_ema.npz", ids=np.array(ids), L=np.where(miss_l[..., None], np.nan, L),
                        R=np.where(miss_r[..., None], np.nan, R), ql=ql, qr=qr, fused=fused, **out)
    print("wrote fuse_ema.npz")


GENERATORS["fuse"] = gen_fuse


def gen_fuse_align():
    """The rest of SURVEY f2: fuse/main_raw.py (Kabsch right->left alignment), fuse/confidence.py
    (weak-perspective reprojection and cross-view consistency confidences) and
    VideoPose3D/fuse/fuse.py (H36M-17 left/right fusion without extrinsics) on synthetic poses with
    missing joints.  The reference functions print diagnostics; stdout is silenced."""
    import contextlib, io
    from fuse.main_raw import _kabsch_rigid_align, _align_right_to_left
    from fuse.confidence import weakpersp_reproj_confidence, crossview_consistency_confidence
    from VideoPose3D.fuse.fuse import fuse_pose_no_extrinsics_h36m

    rng = np.random.default_rng(1)
    out = {}
    # --- Kabsch: 17 COCO joints, right view = rotated + translated left view + noise, NaNs on both sides
    ids = list(range(17))
    J = len(ids)
    A = rng.normal(size=(6, J, 3))
    ang = rng.normal(size=(6, 3))
    Rm = []
    for a in ang:
        cx, sx, cy, sy, cz, sz = np.cos(a[0]), np.sin(a[0]), np.cos(a[1]), np.sin(a[1]), np.cos(a[2]), np.sin(a[2])
        Rm.append(np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
                  @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]))
    Rm = np.stack(Rm)
    Bv = np.einsum("tij,tkj->tki", Rm, A) + rng.normal(size=(6, 1, 3)) + rng.normal(scale=0.01, size=(6, J, 3))
    Bv[5] = -Bv[5]                                   # a reflected frame: exercises the det < 0 branch
    missA = rng.random((6, J)) < 0.15
    missB = rng.random((6, J)) < 0.15
    missA[4] = True; missA[4, :2] = False            # fewer than 3 common joints -> right view returned as is
    A_n = np.where(missA[..., None], np.nan, A)
    B_n = np.where(missB[..., None], np.nan, Bv)
    aligned = np.full((6, J, 3), np.nan)
    rots, trs = [], []
    for t in range(6):
        dl = {j: A_n[t, j] for j in ids if not missA[t, j]}
        dr = {j: B_n[t, j] for j in ids if not missB[t, j]}
        res = _align_right_to_left(dl, dr, ids)
        for j in ids:
            if j in res:
                aligned[t, j] = res[j]
        v = ~missA[t] & ~missB[t]
        if v.sum() >= 3:
            r, tr = _kabsch_rigid_align(B_n[t][v], A_n[t][v])
        else:
            r, tr = np.full((3, 3), np.nan), np.full(3, np.nan)
        rots.append(r); trs.append(tr)
    out.update(kab_left=A_n, kab_right=B_n, kab_aligned=aligned, kab_R=np.stack(rots), kab_t=np.stack(trs))
    # --- confidences (dict inputs in the reference: every joint present, NaN allowed in the values)
    X3 = rng.normal(size=(4, J, 3))
    M = np.linalg.qr(rng.normal(size=(3, 3)))[0][:, :2]
    U2 = 180.0 * (X3 @ M) + np.array([320.0, 240.0]) + rng.normal(scale=4.0, size=(4, J, 2))
    X3[1, 3] = np.nan; U2[2, 5] = np.nan
    conf, err, uhat, ps, pM, pt = [], [], [], [], [], []
    for t in range(4):
        c, e, uh, prm = weakpersp_reproj_confidence({j: X3[t, j] for j in ids}, {j: U2[t, j] for j in ids}, sigma_px=12.0)
        conf.append(c); err.append(e); uhat.append(uh); ps.append(prm["s"]); pM.append(prm["M"]); pt.append(prm["t"])
    out.update(wp_X=X3, wp_U=U2, wp_conf=np.stack(conf), wp_err=np.stack(err), wp_uhat=np.stack(uhat), wp_s=np.array(ps),
               wp_M=np.stack(pM), wp_t=np.stack(pt))
    Xa = rng.normal(size=(4, J, 3))
    Xb = np.einsum("ij,tkj->tki", Rm[0], Xa) * 1.7 + rng.normal(scale=0.05, size=(4, J, 3))
    Xa[2, 9] = np.nan
    Xb[3, 11] = np.nan                                # a key joint missing -> everything NaN / conf 0
    kw = dict(root_idx=0, left_hip_idx=11, right_hip_idx=12, left_shoulder_idx=5, right_shoulder_idx=6)
    cc, dd, xa, xb = [], [], [], []
    for t in range(4):
        for mode in ("hip", "torso"):
            c, d, a_c, b_c, _ = crossview_consistency_confidence({j: Xa[t, j] for j in ids}, {j: Xb[t, j] for j in ids},
                                                                 sigma_3d=0.3, scale_mode=mode, **kw)
            cc.append(c); dd.append(d); xa.append(a_c); xb.append(b_c)
    out.update(cv_A=Xa, cv_B=Xb, cv_conf=np.stack(cc), cv_dist=np.stack(dd), cv_Ac=np.stack(xa), cv_Bc=np.stack(xb))
    # --- VideoPose3D left/right fusion (H36M-17)
    T = 12
    Lh = rng.normal(size=(T, 17, 3))
    Rh = np.einsum("ij,tkj->tki", Rm[1], Lh) + rng.normal(scale=0.04, size=(T, 17, 3)) + rng.normal(size=(T, 1, 3))
    Lh[3, 13] = np.nan; Rh[4, 16] = np.nan; Lh[5, 2] = np.nan; Rh[5, 2] = np.nan
    wl, wr = rng.random((T, 17)), rng.random((T, 17))
    with contextlib.redirect_stdout(io.StringIO()):
        f0, d0 = fuse_pose_no_extrinsics_h36m(Lh, Rh, tau=0.08)
        f1, d1 = fuse_pose_no_extrinsics_h36m(Lh, Rh, tau=0.3, allow_scale=True, mirror_right_x=True, wL=wl, wR=wr)
        f2, _ = fuse_pose_no_extrinsics_h36m(Lh[0], Rh[0], tau=0.5, wL=wl[0], wR=wr[0], return_diagnostics=False)
    out.update(h36_L=Lh, h36_R=Rh, h36_wl=wl, h36_wr=wr, h36_f0=f0, h36_f1=f1, h36_f2=f2,
               h36_gain0=np.array([d["gain"] for d in d0["per_frame"]]), h36_gain1=np.array([d["gain"] for d in d1["per_frame"]]),
               h36_R0=np.stack([d["R"] for d in d0["per_frame"]]), h36_s1=np.array([d["s"] for d in d1["per_frame"]]),
               h36_bad0=np.array(d0["bad_frames"], dtype=np.int64), h36_mean_gain0=np.array(d0["mean_gain"]))
    np.savez_compressed(GOLD / "fuse_align.npz", **out)
    print("wrote fuse_align.npz")


GENERATORS["fuse_align"] = gen_fuse_align


def gen_geometry():
    """The geometry post-processing of the path, from the reference's own functions:
    pose_encoding_to_extri_intri (vggt/vggt/utils/pose_enc.py:62-124), quat_to_mat (utils/rotation.py:14-44),
    unproject_depth_map_to_point_map (utils/geometry.py:15-117), camera_to_world / qrot
    (VideoPose3D/common/camera.py:33-34, quaternion.py:10-24), mpjpe (VideoPose3D/common/loss.py:11-17).
    (vggt/triangulate.py and vggt/multi_view_process.py import cv2 / open3d and cannot be imported here:
    the DLT and the person-origin helpers stay pinned by the oracle's restatement only.)"""
    from VideoPose3D.common.camera import camera_to_world
    from VideoPose3D.common.loss import mpjpe
    from vggt.vggt.utils.geometry import unproject_depth_map_to_point_map
    from vggt.vggt.utils.pose_enc import pose_encoding_to_extri_intri
    from vggt.vggt.utils.rotation import quat_to_mat

    g = torch.Generator().manual_seed(21)
    pe = torch.randn((2, 5, 9), generator=g) * 0.3
    pe[..., 3:7] += torch.tensor([0.0, 0.0, 0.0, 1.0])
    pe[..., 2] += 3.0
    pe[..., 7:] = 0.6 + 0.5 * torch.rand((2, 5, 2), generator=g)
    E, K = pose_encoding_to_extri_intri(pe, (294, 518))
    q = torch.randn((7, 4), generator=g)
    depth = torch.rand((5, 24, 36, 1), generator=g) * 4 + 0.5
    wp = unproject_depth_map_to_point_map(depth.numpy(), E[0].numpy(), K[0].numpy())
    pred = torch.randn((11, 17, 3), generator=g).numpy().astype("float32")
    rot = np.array([0.1407056450843811, -0.1500701755285263, -0.755240797996521, 0.6223280429840088], dtype="float32")
    world = camera_to_world(pred.copy(), R=rot, t=0)
    a, b = torch.randn((4, 9, 17, 3), generator=g), torch.randn((4, 9, 17, 3), generator=g)
    np.savez_compressed(GOLD / "geometry.npz", pose_enc=pe.numpy(), image_hw=np.array([294, 518]), extrinsic=E.numpy(),
                        intrinsic=K.numpy(), quat=q.numpy(), rotmat=quat_to_mat(q).numpy(), depth=depth.numpy(),
                        world_points=wp, cam_pred=pred, cam_rot=rot, cam_world=world, mpjpe_a=a.numpy(), mpjpe_b=b.numpy(),
                        mpjpe=np.array(float(mpjpe(a, b))))
    print("wrote geometry.npz")


GENERATORS["geometry"] = gen_geometry


def gen_formats():
    """a file written by the reference's OWN writer, VideoPose3D/save.py:31-61 `save_3d_joints` (imports
    cleanly here: logging, pathlib, numpy) -- the fused / left / right joints of a clip as one `.npy` holding a dict of
    nested lists -- next to the arrays it was given.  The build's writer (formats.save_3d_joints) must produce the same
    bytes, its reader the same values.  (vggt/save.py and VideoPose3D/run.py import cv2 / trimesh / omegaconf and cannot
    be imported: predictions.npz, the camera NPZ and the pose .npy stay pinned by the cited lines only.)"""
    import importlib.util

    spec = importlib.util.spec_from_file_location("ref_vp3d_save", os.path.join(REF, "VideoPose3D", "save.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    rng = np.random.default_rng(33)
    T = 4
    fused = rng.normal(size=(T, 17, 3))
    left = rng.normal(size=(T, 17, 3)).astype(np.float32)      # float32 inputs: tolist() widens them to Python floats
    right = rng.normal(size=(T, 17, 3))
    fused[1, 5] = np.nan                                       # a missing joint
    right[3, 0, 2] = np.inf
    out = GOLD / "formats_3d_joints.npy"
    mod.save_3d_joints(fused, left, right, out)
    np.savez(GOLD / "formats_3d_joints_inputs.npz", fused=fused, left=left, right=right)
    print("wrote", out.name, out.stat().st_size, "bytes (by the reference's save_3d_joints) + its inputs")


GENERATORS["formats"] = gen_formats


def _ba_clip(T, C, J, seed):
    """A synthetic clip: C cameras on a ring looking at a person near the origin, keypoints = projections + noise."""
    rng = np.random.default_rng(seed)
    K = np.zeros((C, 3, 3))
    K[:, 0, 0], K[:, 1, 1] = rng.uniform(900, 1100, C), rng.uniform(900, 1100, C)
    K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = 960 + rng.normal(0, 5, C), 540 + rng.normal(0, 5, C), 1.0
    R, t = np.zeros((T, C, 3, 3)), np.zeros((T, C, 3))
    for c in range(C):
        a = 2 * np.pi * c / C + 0.3
        ctr = np.array([4 * np.sin(a), -0.3, -4 * np.cos(a)])      # camera centre on the ring
        z = -ctr / np.linalg.norm(ctr)
        x = np.cross([0.0, 1.0, 0.0], z)
        x /= np.linalg.norm(x)
        Rc = np.stack([x, np.cross(z, x), z])
        for s in range(T):
            ang = rng.normal(0, 0.01, 3)
            th = np.linalg.norm(ang)
            Kx = np.array([[0, -ang[2], ang[1]], [ang[2], 0, -ang[0]], [-ang[1], ang[0], 0]])
            dR = np.eye(3) + np.sin(th) / th * Kx + (1 - np.cos(th)) / th**2 * Kx @ Kx
            R[s, c] = dR @ Rc
            t[s, c] = -R[s, c] @ (ctr + rng.normal(0, 0.02, 3))
    X = rng.normal(0, 0.4, (J, 3)) + np.cumsum(rng.normal(0, 0.01, (T, J, 3)), 0)
    Xc = np.einsum("tcij,tkj->tcki", R, X) + t[:, :, None]
    x2d = np.einsum("cij,tckj->tcki", K, Xc / Xc[..., 2:3])[..., :2] + rng.normal(0, 2.0, (T, C, J, 2))
    conf = rng.uniform(0.3, 1.0, (T, C, J))
    Xn = X + rng.normal(0, 0.02, X.shape)
    return K, R, t, Xn, x2d, conf


def _ba_rodrigues(w):
    s = (w * w).sum(-1)[..., None, None]
    small = s < 1e-8
    s_safe = torch.where(small, torch.ones_like(s), s)
    th = torch.sqrt(s_safe)
    A = torch.where(small, 1.0 - s / 6.0 + s * s / 120.0, torch.sin(th) / th)
    B = torch.where(small, 0.5 - s / 24.0 + s * s / 720.0, (1.0 - torch.cos(th)) / s_safe)
    z = torch.zeros_like(w[..., 0])
    Kx = torch.stack([torch.stack([z, -w[..., 2], w[..., 1]], -1), torch.stack([w[..., 2], z, -w[..., 0]], -1),
                      torch.stack([-w[..., 1], w[..., 0], z], -1)], -2)
    return torch.eye(3, dtype=w.dtype) + A * Kx + B * (Kx @ Kx)


def gen_ba():
    """DESIGN §2 "BA": the reference's OWN losses (bundle_adjustment/loss.py, imported by file spec: it needs only
    torch) on two synthetic clips -- each term's value and the autograd gradients of their sum w.r.t. X, R (the matrix)
    and t -- and a 50-step trajectory per mode: those losses, the w wrapper of mode full (R = Exp(w) R0) and
    torch.optim.Adam, as run_local_ba (called at vggt/multi_view_process.py:553-564, defined nowhere) would run them."""
    import importlib.util

    spec = importlib.util.spec_from_file_location("ref_ba_loss", os.path.join(REF, "bundle_adjustment", "loss.py"))
    L = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(L)

    def terms(X, R, t, K, x2d, conf, w=None):
        w = w or {}
        return [L.reprojection_loss(X, R, t, K, x2d, conf, **({"w": w["ba_weight_reproj"]} if w else {})),
                L.camera_smooth_loss(R, t, **({"w": w["ba_weight_smooth"]} if w else {})),
                L.baseline_reg_loss(R, t, **({"w": w["ba_weight_baseline"]} if w else {})),
                L.bone_length_loss(X, **({"w": w["ba_weight_bone_length"]} if w else {})),
                L.pose_temporal_loss(X, **({"w": w["ba_weight_pose_temporal"]} if w else {}))]

    out = {}
    with torch.enable_grad():
        for name, (T, C, J, seed) in {"a": (8, 2, 17, 41), "b": (2, 3, 12, 42)}.items():
            K, R, t, X, x2d, conf = _ba_clip(T, C, J, seed)
            if name == "b":
                X[1, 3] = -(R[1, 2].T @ t[1, 2]) - 0.1 * R[1, 2][2]    # joint 3 of step 1 behind camera 2 (Z clamp)
                conf[:, :, 4] = 0.0                                      # joint 4: conf 0 in every view
            Xt, Rt, tt = (torch.tensor(a, requires_grad=True) for a in (X, R, t))
            tm = terms(Xt, Rt, tt, torch.tensor(K), torch.tensor(x2d), torch.tensor(conf))
            total = tm[0] + tm[1] + tm[2] + tm[3] + tm[4]
            gX, gR, gt = torch.autograd.grad(total, (Xt, Rt, tt))
            for k, v in dict(K=K, R=R, t=t, X=X, x2d=x2d, conf=conf).items():
                out[f"{name}_{k}"] = v
            out[f"{name}_terms"] = np.array([float(v.detach()) for v in tm])
            out[f"{name}_gX"], out[f"{name}_gR"], out[f"{name}_gt"] = gX.numpy(), gR.numpy(), gt.numpy()
        # trajectories on clip a with the configured weights of configs/vggt.yaml:43-51 and lr 1e-2
        wcfg = {"ba_weight_reproj": 1.0, "ba_weight_smooth": 0.1, "ba_weight_baseline": 0.01,
                "ba_weight_bone_length": 0.1, "ba_weight_pose_temporal": 0.1}
        out["traj_weights"] = np.array(list(wcfg.values()))
        out["traj_lr"], out["traj_steps"] = np.array(1e-2), np.array(50)
        Kt, x2dt, conft = (torch.tensor(out[f"a_{k}"]) for k in ("K", "x2d", "conf"))
        R0 = torch.tensor(out["a_R"])
        for mode in ("pose_only", "pose_cam_t", "full"):
            X = torch.tensor(out["a_X"], requires_grad=True)
            t = torch.tensor(out["a_t"], requires_grad=mode != "pose_only")
            w = torch.zeros_like(t, requires_grad=mode == "full")
            params = [X] + ([t] if mode != "pose_only" else []) + ([w] if mode == "full" else [])
            opt = torch.optim.Adam(params, lr=1e-2)
            hist = []
            for _ in range(50):
                opt.zero_grad()
                R = _ba_rodrigues(w) @ R0 if mode == "full" else R0
                tm = terms(X, R, t, Kt, x2dt, conft, wcfg)
                loss = tm[0] + tm[1] + tm[2] + tm[3] + tm[4]
                hist.append([float(loss.detach())] + [float(v.detach()) for v in tm])
                loss.backward()
                opt.step()
            with torch.no_grad():
                R = _ba_rodrigues(w) @ R0 if mode == "full" else R0
            out[f"traj_{mode}_X"], out[f"traj_{mode}_t"] = X.detach().numpy(), t.detach().numpy()
            out[f"traj_{mode}_R"], out[f"traj_{mode}_history"] = R.detach().numpy(), np.array(hist)
    path = GOLD / "ba_losses.npz"
    np.savez_compressed(path, **out)
    print("wrote", path.name, path.stat().st_size, "bytes")


GENERATORS["ba"] = gen_ba


def gen_post_triage():
    """DESIGN §2 "Triage": the reference's OWN post_triage_sequence (triangulation/postprocess.py:125-170, with
    post_triage_single and smooth_skeleton) on a synthetic two-view clip -- X_clean without and with smoothing and the
    per-step reports.  The module imports cv2 and matplotlib at its top and uses neither on this path (dist = None, no
    plots): empty stand-in modules satisfy the two imports when the real ones are not installed."""
    import importlib.util
    import types

    for name in ("cv2", "matplotlib", "matplotlib.pyplot"):
        try:
            __import__(name)
        except ImportError:
            sys.modules[name] = types.ModuleType(name)
    if not hasattr(sys.modules["matplotlib"], "pyplot"):
        sys.modules["matplotlib"].pyplot = sys.modules["matplotlib.pyplot"]
    spec = importlib.util.spec_from_file_location("ref_postprocess", os.path.join(REF, "triangulation", "postprocess.py"))
    P = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(P)

    rng = np.random.default_rng(7)
    Tn, J = 12, 17
    K1 = np.array([[1000.0, 0, 960], [0, 1005, 540], [0, 0, 1]])
    K2 = np.array([[990.0, 0, 950], [0, 1000, 545], [0, 0, 1]])
    a = -0.4
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    T = np.array([2.0, 0.05, 0.4])
    X = rng.normal(size=(J, 3)) * [0.4, 0.8, 0.3] + [0, 0, 6.0] + np.cumsum(rng.normal(scale=0.02, size=(Tn, J, 3)), axis=0)
    X[3, 5] = [0.5, 0.2, -1.0]                 # behind camera 1
    X[4, 6] = R.T @ (np.array([0.1, 0.1, -2.0]) - T)   # 2 m behind camera 2

    def proj(Kc, Rc, tc, Xf):
        p = (Xf @ Rc.T + tc) @ Kc.T
        return p[:, :2] / p[:, 2:3]

    kL = np.stack([proj(K1, np.eye(3), np.zeros(3), X[i]) for i in range(Tn)])
    kR = np.stack([proj(K2, R, T, X[i]) for i in range(Tn)])
    kL += rng.normal(scale=0.6, size=kL.shape) * rng.choice([1.0, 5.0], size=(Tn, J, 1), p=[0.75, 0.25])
    kR += rng.normal(scale=0.6, size=kR.shape)
    kL[7, 2] = np.nan
    cL, cR = rng.uniform(0.2, 1.0, (Tn, J)), rng.uniform(0.2, 1.0, (Tn, J))
    out = dict(X=X, kL=kL, kR=kR, K1=K1, K2=K2, R=R, T=T, confL=cL, confR=cR, conf_thr=np.array(0.3),
               err_thresh_px=np.array(2.0))
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for tag, kw in (("conf", dict(confL=cL, confR=cR)), ("noconf", {})):
            Xc, stats = P.post_triage_sequence(X, kL, kR, K1, K2, R, T, **kw)
            out[f"{tag}_X_clean"] = Xc
            out[f"{tag}_report"] = np.array([[s["rmse_px"], s["median_err_px"], s["pos_depth_ratio"], s["kept_ratio"],
                                              s["kept_count"]] for s in stats])
        out["conf_X_clean_smoothed"] = P.post_triage_sequence(X, kL, kR, K1, K2, R, T, confL=cL, confR=cR, smooth=True,
                                                              sg_win=5)[0]
        out["sg_win"] = np.array(5)
    path = GOLD / "post_triage.npz"
    np.savez_compressed(path, **out)
    print("wrote", path.name, path.stat().st_size, "bytes")


GENERATORS["post_triage"] = gen_post_triage


def gen_scene():
    """DESIGN §2 "Scene cloud": the reference's OWN predictions_to_glb (vggt/visual_util.py:39-236) on a synthetic
    two-view step.  The module imports trimesh, gradio, cv2 and requests at its top; stand-in modules satisfy the
    imports, and the trimesh stand-in records what the function hands it: the vertices and colours of the PointCloud,
    the matrix of Scene.apply_transform, and the radius and height of every creation.cone (scene_scale * 0.05 and
    * 0.1), for which it returns a tiny dummy mesh."""
    import importlib.util
    import json
    import types

    rec = {}

    class Scene:
        def __init__(self):
            self.geometry = []

        def add_geometry(self, g):
            self.geometry.append(g)

        def apply_transform(self, M):
            rec["transform"] = np.array(M, dtype=np.float64)
            return self

    class PointCloud:
        def __init__(self, vertices=None, colors=None):
            rec["vertices"], rec["colors"] = np.array(vertices), np.array(colors)

    class Trimesh:
        def __init__(self, vertices=None, faces=None):
            self.vertices, self.faces = np.asarray(vertices), np.asarray(faces)
            self.visual = types.SimpleNamespace(face_colors=np.zeros((len(self.faces), 4), np.uint8))

    def cone(radius, height, sections=None):
        rec.setdefault("cones", []).append((float(radius), float(height)))
        return Trimesh(np.zeros((3, 3)), np.array([[0, 1, 2]]))

    tm = types.ModuleType("trimesh")
    tm.Scene, tm.PointCloud, tm.Trimesh = Scene, PointCloud, Trimesh
    tm.creation = types.ModuleType("trimesh.creation")
    tm.creation.cone = cone
    saved = {name: sys.modules.get(name) for name in ("trimesh", "trimesh.creation", "gradio", "cv2", "requests")}
    sys.modules["trimesh"], sys.modules["trimesh.creation"] = tm, tm.creation
    for name in ("gradio", "cv2", "requests"):
        sys.modules[name] = types.ModuleType(name)
    try:
        spec = importlib.util.spec_from_file_location("ref_visual_util", os.path.join(REF, "vggt", "visual_util.py"))
        V = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(V)
    finally:
        for name, mod in saved.items():
            if mod is None:
                sys.modules.pop(name, None)
            else:
                sys.modules[name] = mod

    rng = np.random.default_rng(11)
    S, H, Wd = 2, 12, 16
    images = rng.random((S, 3, H, Wd)).astype(np.float32)
    dark, bright = rng.random((S, H, Wd)) < 0.15, rng.random((S, H, Wd)) < 0.15
    for c in range(3):
        images[:, c][dark] = (rng.integers(0, 8, int(dark.sum())) / 255.0 + 0.001).astype(np.float32)    # sums around 16
        images[:, c][bright] = (rng.integers(239, 244, int(bright.sum())) / 255.0 + 0.001).astype(np.float32)   # around 240
    extrinsic = np.zeros((S, 3, 4), np.float32)
    for i in range(S):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        extrinsic[i, :, :3] = q + rng.normal(0, 0.01, (3, 3))
        extrinsic[i, :, 3] = rng.normal(0, 1.5, 3)
    preds = dict(world_points=rng.normal(0, 2, (S, H, Wd, 3)).astype(np.float32),
                 world_points_conf=(1 + np.exp(rng.normal(size=(S, H, Wd)))).astype(np.float32),
                 world_points_from_depth=rng.normal(0, 3, (S, H, Wd, 3)).astype(np.float32),
                 depth_conf=(1 + np.exp(rng.normal(size=(S, H, Wd)))).astype(np.float32), images=images, extrinsic=extrinsic)
    pm = "Predicted Pointmap"
    sets = [dict(conf_thres=50.0, prediction_mode=pm), dict(conf_thres=0.0, prediction_mode=pm),
            dict(conf_thres=10.0, prediction_mode=pm), dict(conf_thres=99.9, prediction_mode=pm),
            dict(conf_thres=50.0, prediction_mode=pm, mask_black_bg=True), dict(conf_thres=50.0, prediction_mode=pm, mask_white_bg=True),
            dict(conf_thres=50.0, prediction_mode="All"), dict(conf_thres=50.0, prediction_mode=pm, filter_by_frames="1:")]
    out = dict(preds, sets_json=np.array(json.dumps(sets)))
    import contextlib
    import io
    for i, kw in enumerate(sets):
        rec.clear()
        with contextlib.redirect_stdout(io.StringIO()):
            V.predictions_to_glb(dict(preds), show_cam=True, **kw)
        cones = np.array(rec["cones"])
        assert (cones == cones[0]).all() and len(cones) == (1 if "filter_by_frames" in kw else S)
        out[f"s{i}_vertices"], out[f"s{i}_colors"] = rec["vertices"], rec["colors"].astype(np.uint8)
        out[f"s{i}_transform"], out[f"s{i}_cone"] = rec["transform"], cones[0]
        assert rec["vertices"].dtype == np.float32 and len(rec["vertices"]) > 0
    path = GOLD / "scene_cloud.npz"
    np.savez_compressed(path, **out)
    print("wrote", path.name, path.stat().st_size, "bytes")


GENERATORS["scene"] = gen_scene


def gen_kinematics():
    """DESIGN §2 "Kinematics": the reference's OWN angle/main.py (imported by file spec with MPLBACKEND=Agg; its plot_angles is
    switched off while it runs, the numbers do not pass through it) on the seeded synthetic skiers of tests/kinematics_cases.py:
    _compute_all_series, compute_series_changes and save_turn_reports, whose turn_metrics.csv and turn_heading.csv are parsed
    back (the csv module writes repr(float): the values round-trip exactly).  Only inputs and results are stored."""
    import csv
    import importlib.util
    import tempfile

    os.environ.setdefault("MPLBACKEND", "Agg")
    sys.path.insert(0, str(ROOT / "tests"))
    import kinematics_cases as kc

    spec = importlib.util.spec_from_file_location("ref_angle_main", os.path.join(REF, "angle", "main.py"))
    A = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(A)
    A.plot_angles = lambda *a, **k: None
    out = {"clips": np.array(list(kc.GOLDEN))}
    for name, case in kc.GOLDEN.items():
        X = case["X"]
        up = np.asarray(case.get("up_axis", (0.0, -1.0, 0.0)), dtype=np.float64)
        joint, body, torso, kdiff, elbow, heading, turns = A._compute_all_series(X, up)
        base = {**joint, **torso, **kdiff, **elbow, **body}
        change = A.compute_series_changes(base)
        report = {**base, **change}
        names = list(report)
        with tempfile.TemporaryDirectory() as tmp:
            import contextlib
            import io
            with contextlib.redirect_stdout(io.StringIO()):
                A.save_turn_reports(Path(tmp), turns, heading, report)
            with open(Path(tmp) / "turn_metrics.csv", newline="") as f:
                rows = list(csv.reader(f))[1:]
            with open(Path(tmp) / "turn_heading.csv", newline="") as f:
                hrows = list(csv.reader(f))[1:]
        stats = np.array([[float(v) for v in r[2:]] for r in rows], dtype=np.float64).reshape(len(turns), len(names), 4)
        assert [r[1] for r in rows[:len(names)]] == names or not turns
        out[f"{name}_X"], out[f"{name}_up"] = X, up
        out[f"{name}_series"] = np.stack([report[n] for n in names])
        out[f"{name}_heading"] = heading
        out[f"{name}_turns"] = np.array([[t[k] for k in ("turn_id", "start_frame", "end_frame", "num_frames", "heading_change_deg",
                                                         "direction")] for t in turns], dtype=np.float64).reshape(len(turns), 6)
        out[f"{name}_stats"] = stats
        out[f"{name}_boundary"] = np.array([int(r[2]) for r in hrows], dtype=np.uint8)
        out["names"] = np.array(names)
        print(f"  {name}: T = {X.shape[0]}, {len(turns)} turns, {int(np.isfinite(heading).sum())} finite headings")
    path = GOLD / "kinematics.npz"
    np.savez_compressed(path, **out)
    print("wrote", path.name, path.stat().st_size, "bytes")


GENERATORS["kinematics"] = gen_kinematics


def gen_evaluate():
    """DESIGN §2 "Evaluation": the reference's OWN VideoPose3D/common/loss.py, VideoPose3D/fuse/fuse_eval.py, metrics/
    unity_data_compare.py (calculate_per_joint_errors, summarize_joint_errors) and metrics/true_data_compare.py
    (compute_temporal_metrics, compute_bone_length_cv), imported by file spec, on the clips of tests/evaluate_cases.py cut to
    their lengths; loss.py in float64, p_mpjpe / n_mpjpe / mpjpe / mean_velocity_error on NaN-free clips only (they return NaN
    or raise otherwise).  `loop_*` is the loop of VideoPose3D/run.py:998-1041 rerun in float64 on lists of clips.  Only
    inputs and results are stored."""
    import hashlib
    import importlib.util
    import warnings

    sys.path.insert(0, str(ROOT / "tests"))
    import evaluate_cases as ec

    def load(name, *parts):
        spec = importlib.util.spec_from_file_location(name, os.path.join(REF, *parts))
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
        return m

    loss = load("ref_loss", "VideoPose3D", "common", "loss.py")
    fe = load("ref_fuse_eval", "VideoPose3D", "fuse", "fuse_eval.py")
    udc = load("ref_unity_data_compare", "metrics", "unity_data_compare.py")
    tdc = load("ref_true_data_compare", "metrics", "true_data_compare.py")
    warnings.simplefilter("ignore")
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a))      # noqa: E731

    def zeroed(g, zr):
        g = g.copy()
        if zr is not None:
            g[:, zr] = 0          # run.py:994
        return g

    def loss_numbers(p, g):
        """mpjpe, p_mpjpe, n_mpjpe, mpjve of a NaN-free clip with extent in every frame"""
        e1 = float(loss.mpjpe(tt(p), tt(g)))
        e3 = float(loss.n_mpjpe(tt(p)[None], tt(g)[None]))
        e2 = float(loss.p_mpjpe(p.copy(), g.copy()))
        ev = float(loss.mean_velocity_error(p, g)) if p.shape[0] >= 2 else float("nan")
        return e1, e2, e3, ev

    out = {"cases": np.array(list(ec.CASES))}
    for name, case in ec.CASES.items():
        for k in ("pred", "target"):      # the inputs are seeded: the large ones are stored as their digest
            a = np.ascontiguousarray(case[k])
            out[f"{name}_{k}"] = a if a.nbytes <= 16384 else np.array(hashlib.sha256(a.tobytes()).hexdigest())
        J = case["pred"].shape[-2]
        lay = ec.layout(J)
        for b, (p, g0) in enumerate(ec.clips_of(case)):
            g = zeroed(g0, case.get("zero_root"))
            n = p.shape[0]
            key = f"{name}_{b}"
            if n >= 1:
                out[f"{key}_mpd"] = np.float64(fe.mean_pairwise_distance(p, g))
                box = udc.init_joint_stat_container(range(J))
                per = np.empty((n, J))
                for t in range(n):
                    e = udc.calculate_per_joint_errors({j: p[t, j] for j in range(J)}, {j: g[t, j] for j in range(J)})
                    udc.accumulate_joint_errors(box, e)
                    per[t] = [e[j] for j in range(J)]
                summ = udc.summarize_joint_errors(box)
                if n <= 41:
                    out[f"{key}_per_joint_err"] = per
                out[f"{key}_joint_summary"] = np.array([[summ[j][k] for k in ("mean", "std", "median", "n")] for j in range(J)], dtype=np.float64)
            clean = bool(n >= 1 and J > 1 and np.isfinite(p).all() and np.isfinite(g).all() and not name.startswith("flat"))
            if clean:
                out[f"{key}_loss"] = np.array(loss_numbers(p, g))
            # the ground-truth-free figures of the prediction
            if len(lay["edges"]):
                out[f"{key}_bone_len"] = fe.bone_lengths(p, np.asarray(lay["edges"], dtype=int)).reshape(n, len(lay["edges"]))
            ts = fe.temporal_stats(p)
            out[f"{key}_p95"] = np.array([ts.get("Speed P95", np.nan), ts.get("Accel P95", np.nan)])
            if J == 17 and n >= 1:
                out[f"{key}_mirror"] = np.float64(fe.symmetry_score_mirror(p[-1]))
            if J == 15:
                seq = [{jid: p[t, i] for i, jid in enumerate(tdc.TARGET_IDS)} for t in range(n)]
                tm = tdc.compute_temporal_metrics(seq)
                out[f"{key}_temporal"] = np.array([tm["speed_mean"], tm["jerk_mean"]], dtype=np.float64)
                out[f"{key}_bone_cv"] = np.float64(tdc.compute_bone_length_cv(seq)) if n else np.float64("nan")
        print(f"  {name}: {list(case['pred'].shape)}")
    for name in ec.FUSED:
        left, right, fused = ec.fused_inputs(name)
        m = fe.eval_fused_pose(left, right, fused)
        out[f"fused_{name}_keys"] = np.array(list(m))
        out[f"fused_{name}_values"] = np.array([m[k] for k in m], dtype=np.float64)
        out[f"fused_{name}_text"] = np.array("Fused Pose Evaluation Metrics:\n" + "".join(f"{k:25s}: {v:.4f}\n" for k, v in m.items()))
    for group, names in ec.EVAL_CLIPS.items():
        tot, N = np.zeros(4), 0
        for nm in names:
            p, g = ec.CASES[nm]["pred"], zeroed(ec.CASES[nm]["target"], 0)
            tot += p.shape[0] * np.array(loss_numbers(p, g))
            N += p.shape[0]
        out[f"loop_{group}"] = tot / N * 1000
    path = GOLD / "evaluate.npz"
    np.savez_compressed(path, **out)
    print("wrote", path.name, path.stat().st_size, "bytes")


GENERATORS["evaluate"] = gen_evaluate


def gen_lens():
    """DESIGN §2 "Lens distortion": the calibration the reference ships (camera_calibration/calibration_parameters.{npz,yml})
    as two small fixtures -- the .yml as it is (settings only) and a pickle-free calibration.npz with camera_matrix,
    dist_coeffs, image_size -- and lens.npz, the outputs of the reference's OWN cv2-free vggt/vggt/dependency/distortion.py
    (apply_distortion on 1, 2 and 4 parameters; iterative_undistortion inside the 4-parameter model's invertible range) on
    the points of tests/lens_cases.py, in float64.  inv_ref_err is the reference's own round-trip error: truth ->
    apply_distortion -> iterative_undistortion against the truth (it stops at a step of 1e-5).  Only inputs and results are
    stored."""
    import importlib.util
    import shutil

    sys.path.insert(0, str(ROOT / "tests"))
    import lens_cases as lc

    src = Path(REF) / "camera_calibration"
    shutil.copyfile(src / "calibration_parameters.yml", GOLD / "calibration_parameters.yml")
    with np.load(src / "calibration_parameters.npz", allow_pickle=False) as z:
        np.savez(GOLD / "calibration.npz", camera_matrix=z["camera_matrix"].astype(np.float64),
                 dist_coeffs=z["dist_coeffs"].astype(np.float64), image_size=z["image_size"].astype(np.int64))
    spec = importlib.util.spec_from_file_location("ref_distortion", os.path.join(REF, "vggt", "vggt", "dependency", "distortion.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))      # noqa: E731
    u, v = lc.ref_forward_points()
    out = {"fwd_u": u, "fwd_v": v}
    for name, params in (("p1", lc.REF_P1), ("p2", lc.REF_P2), ("p4", lc.REF_P4)):
        ud, vd = ref.apply_distortion(tt(params), tt(u), tt(v))
        out[f"fwd_{name}_params"] = params
        out[f"fwd_{name}"] = np.stack([ud.numpy(), vd.numpy()], -1)
    truth = lc.ref_inverse_truth()
    p4 = tt(lc.REF_P4[:1])
    xd, yd = ref.apply_distortion(p4, tt(truth[..., 0]), tt(truth[..., 1]))
    dist_pts = torch.stack([xd, yd], -1)
    und = ref.iterative_undistortion(p4, dist_pts).numpy()
    out |= {"inv_params": lc.REF_P4[:1], "inv_truth": truth, "inv_distorted": dist_pts.numpy(), "inv_undistorted": und,
            "inv_ref_err": np.array(np.abs(und - truth).max())}
    path = GOLD / "lens.npz"
    np.savez_compressed(path, **out)
    print("wrote", path.name, path.stat().st_size, "bytes; the reference's round-trip error:", float(out["inv_ref_err"]))


GENERATORS["lens"] = gen_lens


def gen_bev():
    """DESIGN §2 "Bird's-eye view": the reference's OWN cv2-free functions of front_side/front/bev_utils.py (make_bev_canvas,
    foot_from_bbox_xyxy, image_points_to_bev), front_side/front/run.py (_convert_xywh_to_xyxy, _unnormalize_bbox) and
    front_side/run.py (project_world_to_bev_centered) on seeded inputs, inputs and outputs only.  The modules import cv2,
    tqdm and their sibling loaders at the top and use none of them on these paths: empty stand-in modules satisfy the
    imports.  cv2.findHomography and cv2.warpPerspective are NOT recorded (cv2 is not installed where this runs): they are
    pinned by the restatement and the checks of tests/test_bev_cpu.py."""
    import importlib
    import types

    def stand_in(name, **attrs):
        m = types.ModuleType(name)
        for k, v in attrs.items():
            setattr(m, k, v)
        return m

    nothing = lambda *a, **k: None      # noqa: E731
    fs = os.path.join(REF, "front_side")
    stubs = {
        "front_side": stand_in("front_side", __path__=[fs]),
        "front_side.load": stand_in("front_side.load", load_sam3_results=nothing, load_sam_3d_body_results=nothing),
        "front_side.side": stand_in("front_side.side", __path__=[]),
        "front_side.side.run": stand_in("front_side.side.run", process_side_frame=nothing),
        "front_side.utils": stand_in("front_side.utils", __path__=[]),
        "front_side.utils.merge": stand_in("front_side.utils.merge", merge_frame_to_video=nothing),
        "front_side.side.visualization": stand_in("front_side.side.visualization", __path__=[]),
        "front_side.side.visualization.utils": stand_in("front_side.side.visualization.utils", parse_pose_metainfo=nothing),
    }
    for name in ("cv2", "tqdm"):
        try:
            __import__(name)
        except ImportError:
            stubs[name] = stand_in(name, tqdm=lambda it, **k: it)
    saved = {name: sys.modules.get(name) for name in stubs}
    sys.modules.update(stubs)
    try:
        bu = importlib.import_module("front_side.front.bev_utils")
        fr = importlib.import_module("front_side.front.run")
        top = importlib.import_module("front_side.run")
    finally:
        for name, mod in saved.items():
            if mod is None:
                sys.modules.pop(name, None)
            else:
                sys.modules[name] = mod
        for name in [n for n in sys.modules if n == "front_side" or n.startswith("front_side.")]:
            sys.modules.pop(name, None)

    rng = np.random.default_rng(11)
    out = {}
    cfgs = np.array([[30.0, 60.0, 20.0, 5.0, 10.0], [12.5, 33.3, 7.5, 1.25, 0.7], [30.0, 60.0, 0.9, 5.0, 10.0]])
    sizes, mats = [], []
    for c in cfgs:
        size, S = bu.make_bev_canvas(bu.BeVConfig(*map(float, c)))
        sizes.append(size), mats.append(S)
    out |= {"canvas_cfg": cfgs, "canvas_size": np.array(sizes, np.int64), "canvas_S": np.array(mats)}
    boxes = rng.uniform(0, 1000, (9, 4))
    out |= {"foot_boxes": boxes, "foot_out": np.stack([bu.foot_from_bbox_xyxy(b) for b in boxes])}
    H = np.array([[0.96, 0.81, -920.0], [0.01, -3.7, 4008.0], [1e-5, 0.00268, 1.0]])
    uv = rng.uniform([0, 150], [1920, 1080], (33, 2))
    out |= {"pts_H": H, "pts_uv": uv, "pts_out": bu.image_points_to_bev(uv, H)}
    xywh = rng.uniform(0, 0.5, (7, 4))
    xyxy = fr._convert_xywh_to_xyxy(xywh)
    out |= {"xywh": xywh, "xyxy": xyxy, "unnorm_size": np.array([1080, 1920], np.int64),
            "unnorm_out": fr._unnormalize_bbox(xyxy, (1080, 1920))}
    # the skeleton on the plan: seeded joints with NaN joints; a 1/8 m grid at 0.25 m / px meets exact halves
    cases = []
    for k, (mpp, grid, rot, axes) in enumerate(((0.02, False, True, (0, 2)), (0.25, True, True, (0, 2)), (0.25, True, False, (0, 2)),
                                                 (0.02, False, False, (0, 1)), (0.5, True, True, (2, 1)))):
        J = 21 if k % 2 == 0 else 17
        X = rng.integers(-40, 41, (J, 3)).astype(np.float64) / 8.0 if grid else rng.normal(size=(J, 3)) + [0.5, 1.0, 6.0]
        X[3] = np.nan
        X[7, 1] = np.nan
        center_world = np.array([0.125, -0.25, 0.375]) if grid else np.nanmean(X, axis=0)
        center_px = (int(rng.integers(100, 700)), int(rng.integers(100, 1500)))
        pts = top.project_world_to_bev_centered(X, center_world, center_px, mpp, use_axes=axes, rot90_left=rot)
        valid = np.array([p is not None for p in pts])
        px = np.array([p if p is not None else (0, 0) for p in pts], np.int64)
        cases.append((X, center_world, np.array(center_px, np.int64), np.array(mpp), np.array(axes, np.int64), np.array(rot), px, valid))
    for k, vals in enumerate(cases):
        for key, v in zip(("X", "center_world", "center_px", "mpp", "axes", "rot", "px", "valid"), vals):
            out[f"skel{k}_{key}"] = v
    out["skel_count"] = np.array(len(cases))
    path = GOLD / "bev.npz"
    np.savez_compressed(path, **out)
    print("wrote", path.name, path.stat().st_size, "bytes")


GENERATORS["bev"] = gen_bev


def gen_calibrate():
    """DESIGN §2 "Calibration": recorded results of the calibration the reference ships (camera_calibration/
    calibration_parameters.npz): its camera matrix, its first eight coefficients, the frame size and 24 of its 181 board
    poses (indices linspace(0, 180, 24) truncated), with the board's geometry (9 x 6 inner corners, squares of 25).  The tests
    synthesise corners from these by projecting the board.  The file's pickled object arrays are never touched."""
    with np.load(Path(REF) / "camera_calibration" / "calibration_parameters.npz", allow_pickle=False) as z:
        idx = np.linspace(0, 180, 24).astype(np.int64)
        out = {"camera_matrix": z["camera_matrix"].astype(np.float64), "dist_coeffs": z["dist_coeffs"].astype(np.float64).reshape(-1)[:8],
               "image_size": z["image_size"].astype(np.int64), "rvecs": z["rvecs"].astype(np.float64).reshape(-1, 3)[idx],
               "tvecs": z["tvecs"].astype(np.float64).reshape(-1, 3)[idx], "view_index": idx,
               "board": np.array([9, 6], np.int64), "square": np.array(25.0)}
    path = GOLD / "calibrate.npz"
    np.savez_compressed(path, **out)
    print("wrote", path.name, path.stat().st_size, "bytes")


GENERATORS["calibrate"] = gen_calibrate


def gen_fuse_group():
    """DESIGN §2 "Joint quality", "Group fusion", "Skeleton conversion": the reference's OWN fuse/fuse.py (no-GT quality:
    estimate_bone_median_lengths, q_from_bone_deviation, q_from_temporal, q_2d_sanity, compute_q_nogt_frame,
    body_side_bias), fuse/main_unity.py (_fuse_pair, then temporal_smooth_ema and fuse/save.py's array form, for every pair
    of three views) and VideoPose3D/coco_hm36.py on seeded synthetic clips.  Inputs and results only."""
    import itertools
    import warnings
    sys.path.insert(0, str(ROOT / "tests"))
    import fuse_group_cases as gc
    from fuse import fuse as rf
    from fuse.main_unity import _fuse_pair, TARGET_IDS, UNITY_MHR70_MAPPING
    from fuse.save import _seq_dicts_to_array
    from metrics.true_data_compare import BONE_EDGES
    from VideoPose3D import coco_hm36 as rc

    out = {"target_ids": np.array(TARGET_IDS, np.int64), "bone_edge_ids": np.array(BONE_EDGES, np.int64)}
    ids = list(TARGET_IDS)
    # --- quality: one view's clip, dicts without the missing joints
    c = gc.quality_golden_case()
    X, U, W, H = c["X"], c["U"], c["width"], c["height"]
    edge_ids = [(gc.id_of(a), gc.id_of(b)) for a, b in c["edges"]]
    T, J = X.shape[:2]
    seq3 = [{jid: X[t, j] for j, jid in enumerate(ids) if np.isfinite(X[t, j]).all()} for t in range(T)]
    seq2 = [{jid: U[t, j] for j, jid in enumerate(ids) if j not in c["u_absent"]} for t in range(T)]
    assert all(seq3)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                      # nanmedian of the edge that is never seen
        med = rf.estimate_bone_median_lengths(seq3, ids, edge_ids)
    qb = np.stack([rf.q_from_bone_deviation(seq3[t], ids, edge_ids, med) for t in range(T)])
    qt = np.stack([rf.q_from_temporal(seq3[t - 1] if t else None, seq3[t], ids, beta=c["beta_temp"]) for t in range(T)])
    qs = np.stack([rf.q_2d_sanity(seq2[t], ids, W, H) for t in range(T)])
    kw = dict(beta_temp=c["beta_temp"], w_bone=c["w_bone"], w_temp=c["w_temp"], w_san=c["w_san"])
    q = np.stack([rf.compute_q_nogt_frame(seq3[t], seq3[t - 1] if t else None, seq2[t], ids, edge_ids, med, W, H, **kw) for t in range(T)])
    q_noU = np.stack([rf.compute_q_nogt_frame(seq3[t], seq3[t - 1] if t else None, None, ids, edge_ids, med, W, H, **kw) for t in range(T)])
    out |= {"q_med": med, "q_bone": qb, "q_temp": qt, "q_san": qs, "q": q, "q_noU": q_noU,
            "side_bias": rf.body_side_bias(ids, UNITY_MHR70_MAPPING, 0.75)}
    # --- group: three views, every pair by main_unity._fuse_pair, then the EMA and save.py's array
    g = gc.group_golden_case()
    P3, P2 = g["X"], g["U"]
    seqs = [[{"p2d": {jid: P2[v, t, j] for j, jid in enumerate(ids)}, "p3d": {jid: P3[v, t, j] for j, jid in enumerate(ids)}}
             for t in range(P3.shape[1])] for v in range(P3.shape[0])]
    fused, smoothed = [], []
    for a, b in itertools.combinations(range(P3.shape[0]), 2):
        fs = _fuse_pair(seqs[a], seqs[b], sigma_px=g["sigma_px"], sigma_3d=g["sigma_3d"])
        fused.append(_seq_dicts_to_array(fs, ids))
        smoothed.append(_seq_dicts_to_array(rf.temporal_smooth_ema(fs, ids, **g["ema"]), ids))
    out |= {"g_fused": np.stack(fused), "g_smoothed": np.stack(smoothed), "g_X": P3, "g_U": P2, "q_X": X, "q_U": U,
            "q_edges": np.array(c["edges"], np.int64)}
    # --- skeleton conversion
    for name, arr in gc.skeleton_golden_inputs().items():
        out[f"sk_{name}"] = arr
        if name.startswith("coco"):
            out[f"sk_{name}_h36m"] = rc.coco_to_h36m(arr)
            out[f"sk_{name}_h36m_nohead"] = rc.coco_to_h36m(arr, synthesize_head=False)
        else:
            out[f"sk_{name}_coco"] = rc.h36m_to_coco(arr)
            out[f"sk_{name}_coco_face"] = rc.h36m_to_coco(arr, synthesize_face=True)
    path = GOLD / "fuse_group.npz"
    np.savez_compressed(path, **out)
    print("wrote", path.name, path.stat().st_size, "bytes")


GENERATORS["fuse_group"] = gen_fuse_group


def gen_masks():
    """DESIGN §2 "Masks": the reference's OWN masks_to_boxes and mask_iou (prepare_front_results/sam3/perflib/masks_ops.py) and
    generic_nms_cpu (perflib/nms.py) on the CPU, on the inputs of tests/masks_cases.py.  The sam3 package's __init__ imports
    iopath, which is not installed: an empty stand-in package with the real path takes its place, everything below it
    (sam3.perflib and its modules) is the reference's own.  The NMS problems have distinct scores: the CPU loop leaves ties to
    argsort.  Only inputs and results are stored.  (connected_components_cpu needs skimage and the _slow point sampler cv2:
    neither is installed, so they have no golden.)"""
    import hashlib
    import types

    sys.path.insert(0, str(ROOT / "tests"))
    import masks_cases as mc

    pkg = types.ModuleType("sam3")
    pkg.__path__ = [os.path.join(REF, "prepare_front_results", "sam3")]
    saved = sys.modules.get("sam3")
    sys.modules["sam3"] = pkg
    try:
        from sam3.perflib import masks_ops, nms
    finally:
        if saved is None:
            sys.modules.pop("sam3", None)
        else:
            sys.modules["sam3"] = saved
    out = {}
    H, W = mc.SIZES[0]
    for k, (n, m) in enumerate(mc.IOU_SHAPES):
        a, b = mc.iou_masks(n, H, W, seed=100 + k), mc.iou_masks(m, H, W, seed=200 + k)
        out[f"iou{k}_a"], out[f"iou{k}_b"] = a, b
        out[f"iou{k}_iou"] = masks_ops.mask_iou(torch.from_numpy(a != 0), torch.from_numpy(b != 0)).numpy()
        out[f"iou{k}_boxes"] = masks_ops.masks_to_boxes(torch.from_numpy(a), list(range(n))).numpy()
    for n in mc.NMS_COUNTS:
        io, scores, _ = mc.nms_problem(n, seed=300 + n)
        assert len(np.unique(scores)) == n
        # the inputs are seeded: stored as their digest
        out[f"nms{n}_digest"] = np.array(hashlib.sha256(io.tobytes() + scores.tobytes()).hexdigest())
        for thr in mc.NMS_THRESHOLDS:
            out[f"nms{n}_kept_{thr}"] = nms.generic_nms_cpu(torch.from_numpy(io), torch.from_numpy(scores), thr).numpy()
    path = GOLD / "masks.npz"
    np.savez_compressed(path, **out)
    print("wrote", path.name, path.stat().st_size, "bytes")


GENERATORS["masks"] = gen_masks


def gen_assign():
    """DESIGN §2 "Association and tracking": the reference's OWN associate_det_trk (prepare_front_results/sam3/perflib/
    associate_det_trk.py: mask_iou, scipy's linear_sum_assignment and its Python loops) on the CPU, on the mask sets of
    tests/assign_cases.py.  The sam3 package's __init__ imports iopath, which is not installed: the empty stand-in package of
    gen_masks takes its place, everything below it is the reference's own.  Only a digest of the seeded inputs and the four
    results are stored: the new detections and unmatched tracks as flags, det_to_matched_trk as a [N, M] mask, and
    matched_det_scores as [M, 2] float64 rows (NaN: the track has no entry) with the entries' order of insertion."""
    import hashlib
    import types

    sys.path.insert(0, str(ROOT / "tests"))
    import assign_cases as ac

    pkg = types.ModuleType("sam3")
    pkg.__path__ = [os.path.join(REF, "prepare_front_results", "sam3")]
    saved = sys.modules.get("sam3")
    sys.modules["sam3"] = pkg
    try:
        from sam3.perflib.associate_det_trk import associate_det_trk
    finally:
        if saved is None:
            sys.modules.pop("sam3", None)
        else:
            sys.modules["sam3"] = saved
    out = {}
    for name in ac.ASSOC_CASES:
        det, trk, scores = ac.assoc_case(name)
        N, M = len(det), len(trk)
        thr = ac.ASSOC_THRESHOLDS
        new, unmatched, det_to_trk, det_scores = associate_det_trk(
            torch.from_numpy(det), torch.from_numpy(trk), thr["iou_threshold"], thr["iou_threshold_trk"], torch.from_numpy(scores),
            thr["new_det_thresh"])
        out[f"{name}_digest"] = np.array(hashlib.sha256(det.tobytes() + trk.tobytes() + scores.tobytes()).hexdigest())
        out[f"{name}_new"] = np.isin(np.arange(N), new)
        out[f"{name}_unmatched"] = np.isin(np.arange(M), unmatched)
        out[f"{name}_det_trk"] = np.array([[t in det_to_trk.get(d, []) for t in range(M)] for d in range(N)], dtype=bool)
        rows = np.full((M, 2), np.nan)
        for t, pair in det_scores.items():
            rows[int(t)] = pair
        out[f"{name}_scores"] = rows
        out[f"{name}_score_order"] = np.array([int(t) for t in det_scores], dtype=np.int32)
    path = GOLD / "assign.npz"
    np.savez_compressed(path, **out)
    print("wrote", path.name, path.stat().st_size, "bytes")


GENERATORS["assign"] = gen_assign


if __name__ == "__main__":
    which = sys.argv[1:] or list(GENERATORS)
    for w in which:
        GENERATORS[w]()
