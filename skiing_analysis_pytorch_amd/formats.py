"""On-disk formats either side of the hot path.

Input: the per-clip `.pt` written by the reference's prepare_dataset stage
(prepare_dataset/main.py:53-98, process/preprocess.py:160-171):
    {video_name, video_path, frame_count, img_shape, fps,
     detectron2: {bbox [T,4] | [T,N,4], keypoints [T,17,2|3], keypoints_score [T,17]}, yolo: {...}, depth?, frames?}
read as the reference's loaders do (vggt/load.py:268-370 `load_info`,
VideoPose3D/common/custom_dataset.py:106-164), minus the video decode: torchvision / PyAV are
not part of this build, so frames come from the `.pt` itself when present or from the caller.

Output: `.npy [T,17,3]` of the lifter (VideoPose3D/run.py:1089-1092), the camera NPZ of the
VGGT stage (vggt/save.py:84-110, `infer.save_camera_info`) and the per-step scene GLB as a point cloud
(vggt/save.py:58-73; `write_glb_points` / `read_glb_points`, a minimal glTF-2.0 binary of this package's own).
"""
from __future__ import annotations

from dataclasses import dataclass
from pathlib import Path
from typing import Optional, Tuple

import numpy as np
import torch


def _load_pt(path) -> dict:
    # only loaders that execute nothing from the file
    return torch.load(str(path), map_location="cpu", weights_only=True)


def _to_numpy_xy(kpts) -> np.ndarray:
    a = kpts.detach().cpu().numpy() if isinstance(kpts, torch.Tensor) else np.asarray(kpts)
    return a[..., :2].astype(np.float32)


def read_video_frames(video_file_path) -> torch.Tensor:
    """[T, H, W, 3] uint8 RGB frames of a video file, as the reference's
    `read_video(path, pts_unit="sec", output_format="THWC")[0]` (vggt/load.py:292).  Video decode is
    outside this build: an installed torchvision / OpenCV is used when there is one, and the
    error says what to do otherwise."""
    try:
        from torchvision.io import read_video   # the reference's own decoder
        return read_video(str(video_file_path), pts_unit="sec", output_format="THWC")[0]
    except ImportError:
        pass
    try:
        import cv2
    except ImportError:
        raise RuntimeError(f"no video decoder in this environment (torchvision / cv2) for {video_file_path}: embed the "
                           "frames in the .pt file (key 'frames', [T,H,W,3] uint8, as prepare_dataset can) or pass frames=")
    cap, out = cv2.VideoCapture(str(video_file_path)), []
    while True:
        ok, fr = cap.read()
        if not ok:
            break
        out.append(torch.from_numpy(cv2.cvtColor(fr, cv2.COLOR_BGR2RGB)))
    cap.release()
    return torch.stack(out)


def load_info(pt_file_path, frames: Optional[torch.Tensor] = None, assume_normalized: Optional[bool] = None,
              clip_bbox_to_image: bool = True, dtype=np.float32, video_file_path=None
              ) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray, Optional[torch.Tensor]]:
    """vggt/load.py:268-370.  Returns (keypoints_xy [T,K,2] pixels, keypoints_score [T,K],
    bboxes_xyxy [T,4|N,4] pixels, bbox_scores, frames [T,H,W,3] uint8 | None).  Frames: the `frames`
    argument, else the `.pt` file's own `frames`, else decoded from `video_file_path` when a decoder is
    installed (the reference always decodes the video)."""
    data = _load_pt(pt_file_path)
    if "detectron2" not in data:
        raise KeyError(f"pt file missing 'detectron2' root: {pt_file_path}")
    d2 = data["detectron2"]
    if frames is None and "frames" in data and data["frames"] is not None:
        frames = data["frames"]
    if frames is None and video_file_path is not None and Path(video_file_path).exists():
        frames = read_video_frames(video_file_path)
    if frames is not None:
        H, W = int(frames.shape[1]), int(frames.shape[2])
    elif "img_shape" in data:
        H, W = int(data["img_shape"][0]), int(data["img_shape"][1])
    else:
        raise KeyError("neither frames nor img_shape available to de-normalise the keypoints")
    if "keypoints" not in d2:
        raise KeyError(f"pt file missing detectron2.keypoints: {pt_file_path}")
    kpts_t = d2["keypoints"]
    kpts_xy = _to_numpy_xy(kpts_t)
    mx = np.nanmax(kpts_xy) if kpts_xy.size else 0.0
    if assume_normalized is True or (assume_normalized is None and mx <= 1.5):
        kpts_xy = kpts_xy * np.array([W, H], dtype=np.float32)
    if "keypoints_score" in d2:
        kpt_scores = np.asarray(d2["keypoints_score"].detach().cpu().numpy() if isinstance(d2["keypoints_score"], torch.Tensor) else d2["keypoints_score"])
    elif kpts_t.shape[-1] >= 3:
        kpt_scores = np.asarray(kpts_t[..., 2])
    else:
        kpt_scores = np.ones(kpts_xy.shape[:2], dtype=dtype)
    if kpts_xy.ndim != 3 or kpts_xy.shape[2] != 2:
        raise ValueError(f"Invalid D2 keypoints shape after processing: {kpts_xy.shape}")
    if kpt_scores.shape != kpts_xy.shape[:2]:
        raise ValueError(f"D2 keypoints_score shape {kpt_scores.shape} mismatches keypoints {kpts_xy.shape}")
    if "bbox" not in d2:
        raise KeyError(f"pt file missing detectron2.bbox: {pt_file_path}")
    bb = d2["bbox"]
    bboxes = (bb.detach().cpu().numpy() if isinstance(bb, torch.Tensor) else np.asarray(bb)).astype(dtype, copy=True)
    mxb = np.nanmax(bboxes) if bboxes.size else 0.0
    if assume_normalized is True or (assume_normalized is None and mxb <= 1.5):
        bboxes[..., 0::2] *= float(W)
        bboxes[..., 1::2] *= float(H)
    if "scores" in d2:
        bbox_scores = np.asarray(d2["scores"], dtype=dtype)
    elif "bbox_score" in d2:
        bbox_scores = np.asarray(d2["bbox_score"], dtype=dtype)
    else:
        bbox_scores = np.ones(bboxes.shape[:-1], dtype=dtype)
    if clip_bbox_to_image:
        x1 = np.minimum(bboxes[..., 0], bboxes[..., 2]); x2 = np.maximum(bboxes[..., 0], bboxes[..., 2])
        y1 = np.minimum(bboxes[..., 1], bboxes[..., 3]); y2 = np.maximum(bboxes[..., 1], bboxes[..., 3])
        bboxes = np.stack([np.clip(x1, 0, W - 1), np.clip(y1, 0, H - 1), np.clip(x2, 0, W - 1), np.clip(y2, 0, H - 1)], axis=-1)
    return (kpts_xy.astype(dtype, copy=False), kpt_scores.astype(dtype, copy=False), bboxes.astype(dtype, copy=False),
            bbox_scores.astype(dtype, copy=False), frames)


def save_pose_npy(path, prediction: np.ndarray) -> Path:
    """VideoPose3D/run.py:1089-1092: `<video>.npy` holding [T, 17, 3] float32 camera-space joints."""
    p = Path(path)
    p.parent.mkdir(parents=True, exist_ok=True)
    np.save(p, np.asarray(prediction, dtype=np.float32))
    return p if p.suffix == ".npy" else p.with_suffix(p.suffix + ".npy")


def save_3d_joints(fused_joints_3d: np.ndarray, left_joints_3d: np.ndarray, right_joints_3d: np.ndarray, save_path,
                   fmt: str = "npy") -> Path:
    """VideoPose3D/save.py:31-61: one `.npy` holding a dict of nested lists
    {"fused_joints_3d", "left_joints_3d", "right_joints_3d"} (an object array, i.e. a pickle: readers use
    `np.load(path, allow_pickle=True).item()`).  Any other `fmt` raises ValueError like the reference."""
    if fmt != "npy":
        raise ValueError(f"Unsupported format: {fmt}")
    p = Path(save_path)
    p.parent.mkdir(parents=True, exist_ok=True)
    payload = {
        "fused_joints_3d": np.asarray(fused_joints_3d).tolist(),
        "left_joints_3d": np.asarray(left_joints_3d).tolist(),
        "right_joints_3d": np.asarray(right_joints_3d).tolist(),
    }
    np.save(p, payload)
    return p if p.suffix == ".npy" else p.with_suffix(p.suffix + ".npy")


def load_3d_joints(path) -> dict:
    """Reader of `save_3d_joints` files written by THIS package (unpickles: never point it at a file of
    unknown origin).  -> dict of float64 arrays."""
    d = np.load(Path(path), allow_pickle=True).item()
    return {k: np.asarray(d[k], dtype=np.float64) for k in ("fused_joints_3d", "left_joints_3d", "right_joints_3d")}


def save_predictions_npz(outdir, preds: dict) -> Path:
    """vggt/save.py:52-56: `<outdir>/predictions.npz` = np.savez of every array of the prediction dict
    (device tensors are brought to the host; None entries, e.g. pose_enc_list, are skipped as np.savez
    cannot hold them without pickling)."""
    out = Path(outdir)
    out.mkdir(parents=True, exist_ok=True)
    arrays = {}
    for k, v in preds.items():
        if v is None:
            continue
        if isinstance(v, torch.Tensor):
            v = v.detach().cpu().numpy()
        arrays[k] = np.asarray(v)
    np.savez(out / "predictions.npz", **arrays)
    return out / "predictions.npz"


# ---- GLB point clouds (glTF 2.0 binary; the scene file of vggt/save.py:58-73, points only) ----
_GLB_MAGIC, _GLB_JSON, _GLB_BIN = 0x46546C67, 0x4E4F534A, 0x004E4942


def write_glb_points(path, xyz, rgb) -> Path:
    """A coloured point cloud as a minimal glTF-2.0 binary: one mesh, one primitive of mode 0 (POINTS); POSITION float32
    VEC3 with the `min` / `max` the specification requires (taken over the finite coordinates: JSON cannot hold NaN or
    inf), COLOR_0 normalised unsigned-byte VEC4 with alpha 255.  The JSON chunk is padded with spaces and the BIN chunk
    with zeros to 4 bytes.  xyz [N, 3], rgb [N, 3] uint8; an empty cloud is written as the reference's single white point
    (1, 0, 0) (vggt/visual_util.py:194-196).  The bytes are this writer's own, not trimesh's."""
    import json
    import struct

    xyz = np.ascontiguousarray(np.asarray(xyz, dtype=np.float32).reshape(-1, 3))
    rgb = np.asarray(rgb, dtype=np.uint8).reshape(-1, 3)
    if len(xyz) != len(rgb):
        raise ValueError(f"write_glb_points: {len(xyz)} vertices but {len(rgb)} colours")
    if len(xyz) == 0:
        xyz = np.array([[1.0, 0.0, 0.0]], np.float32)
        rgb = np.array([[255, 255, 255]], np.uint8)
    n = len(xyz)
    rgba = np.full((n, 4), 255, np.uint8)
    rgba[:, :3] = rgb
    lo, hi = [], []
    for a in range(3):
        col = xyz[:, a][np.isfinite(xyz[:, a])]
        lo.append(float(col.min()) if col.size else 0.0)
        hi.append(float(col.max()) if col.size else 0.0)
    gltf = {
        "asset": {"version": "2.0", "generator": "skiing_analysis_pytorch_amd"},
        "scene": 0,
        "scenes": [{"nodes": [0]}],
        "nodes": [{"mesh": 0}],
        "meshes": [{"primitives": [{"attributes": {"POSITION": 0, "COLOR_0": 1}, "mode": 0}]}],
        "accessors": [
            {"bufferView": 0, "componentType": 5126, "count": n, "type": "VEC3", "min": lo, "max": hi},
            {"bufferView": 1, "componentType": 5121, "normalized": True, "count": n, "type": "VEC4"},
        ],
        "bufferViews": [
            {"buffer": 0, "byteOffset": 0, "byteLength": 12 * n, "target": 34962},
            {"buffer": 0, "byteOffset": 12 * n, "byteLength": 4 * n, "target": 34962},
        ],
        "buffers": [{"byteLength": 16 * n}],
    }
    js = json.dumps(gltf, separators=(",", ":")).encode("utf-8")
    js += b" " * (-len(js) % 4)
    blob = xyz.astype("<f4").tobytes() + rgba.tobytes()
    blob += b"\0" * (-len(blob) % 4)
    total = 12 + 8 + len(js) + 8 + len(blob)
    p = Path(path)
    with open(p, "wb") as f:
        f.write(struct.pack("<III", _GLB_MAGIC, 2, total))
        f.write(struct.pack("<II", len(js), _GLB_JSON))
        f.write(js)
        f.write(struct.pack("<II", len(blob), _GLB_BIN))
        f.write(blob)
    return p


def read_glb_points(path) -> Tuple[np.ndarray, np.ndarray]:
    """Reader of the point clouds `write_glb_points` writes -> (xyz float32 [N, 3], rgb uint8 [N, 3]).  It follows the
    accessors of the first primitive (float32 VEC3 POSITION, unsigned-byte VEC3 / VEC4 COLOR_0, tightly packed or strided
    views of the one embedded buffer); anything else is a ValueError."""
    import json
    import struct

    data = Path(path).read_bytes()
    if len(data) < 20 or struct.unpack_from("<I", data, 0)[0] != _GLB_MAGIC:
        raise ValueError(f"{path}: not a GLB file")
    version, total = struct.unpack_from("<II", data, 4)
    if version != 2 or total != len(data):
        raise ValueError(f"{path}: GLB version {version}, length {total} in a file of {len(data)} bytes")
    chunks, off = {}, 12
    while off + 8 <= total:
        size, kind = struct.unpack_from("<II", data, off)
        chunks.setdefault(kind, data[off + 8:off + 8 + size])
        off += 8 + size
    if _GLB_JSON not in chunks or _GLB_BIN not in chunks:
        raise ValueError(f"{path}: needs a JSON and a BIN chunk")
    gltf, blob = json.loads(chunks[_GLB_JSON].decode("utf-8")), chunks[_GLB_BIN]
    prim = gltf["meshes"][0]["primitives"][0]
    if prim.get("mode", 4) != 0:
        raise ValueError(f"{path}: the first primitive is not a point list")

    def view(index, dtype, width_ok):
        acc = gltf["accessors"][index]
        bv = gltf["bufferViews"][acc["bufferView"]]
        width = {"VEC3": 3, "VEC4": 4}.get(acc["type"])
        if acc["componentType"] != {"<f4": 5126, "u1": 5121}[dtype] or width not in width_ok:
            raise ValueError(f"{path}: accessor {index} is {acc['componentType']} {acc['type']}")
        item = np.dtype(dtype).itemsize * width
        stride = bv.get("byteStride", item)
        start = bv.get("byteOffset", 0) + acc.get("byteOffset", 0)
        count = acc["count"]
        if count and start + (count - 1) * stride + item > len(blob):
            raise ValueError(f"{path}: accessor {index} runs past the buffer")
        rows = np.frombuffer(blob, np.uint8, offset=start, count=(count - 1) * stride + item if count else 0)
        rows = np.lib.stride_tricks.as_strided(rows, (count, item), (stride, 1)) if count else rows.reshape(0, item)
        return np.ascontiguousarray(rows).view(dtype).reshape(count, width)

    xyz = view(prim["attributes"]["POSITION"], "<f4", (3,)).astype(np.float32)
    rgb = view(prim["attributes"]["COLOR_0"], "u1", (3, 4))[:, :3].copy()
    return xyz, rgb


# ---- camera calibration files (camera_calibration/calibration_parameters.{npz,yml}) ---------------------------------------
@dataclass(frozen=True)
class Calibration:
    """One camera's calibration as camera_calibration writes it."""
    K: np.ndarray               # float64 [3, 3]
    dist: np.ndarray            # float64 [14]: k1 k2 p1 p2 k3 k4 k5 k6 s1 s2 s3 s4 tx ty (OpenCV's order), zero-padded
    image_size: Tuple[int, int]  # (width, height) of the frames it was solved on

    def scaled_to(self, width: int, height: int) -> "Calibration":
        """The same lens on frames of another size with the same aspect ratio: fx, cx scale with the width, fy, cy with the
        height; the coefficients act on normalised coordinates and stay as they are.  Another aspect ratio means a crop or an
        anamorphic resize that the file does not describe, and is refused."""
        w0, h0 = self.image_size
        width, height = int(width), int(height)
        if width < 1 or height < 1 or width * h0 != height * w0:
            raise ValueError(f"calibration of {w0} x {h0} frames cannot be rescaled to {width} x {height}: another aspect ratio")
        K = self.K.copy()
        K[0, 0] *= width / w0
        K[0, 2] *= width / w0
        K[1, 1] *= height / h0
        K[1, 2] *= height / h0
        return Calibration(K, self.dist.copy(), (width, height))


def _opencv_yaml(text: str) -> dict:
    """The subset of OpenCV's FileStorage YAML that calibration files use: `key: scalar` lines and `key: !!opencv-matrix`
    nodes (rows, cols, dt, data: [ ... ] over several lines), after the `%YAML:1.0` header.  Parsed by hand: the header is
    not valid YAML 1.1, and the package does not depend on a YAML library."""
    import re

    if not text.lstrip().startswith("%YAML"):
        raise ValueError("not an OpenCV YAML file (no %YAML header)")
    out = {}
    for m in re.finditer(r"^(\w+):[ \t]*!!opencv-matrix\s*\n((?:[ \t]+.*\n?)+)", text, flags=re.M):
        body = m.group(2)
        rows, cols = (int(re.search(rf"^\s+{k}:\s*(\d+)", body, flags=re.M).group(1)) for k in ("rows", "cols"))
        dt = re.search(r"^\s+dt:\s*\"?(\w+)\"?", body, flags=re.M).group(1)
        data = re.search(r"data:\s*\[(.*?)\]", body, flags=re.S)
        if dt not in ("d", "f", "i") or data is None:
            raise ValueError(f"opencv-matrix {m.group(1)}: unsupported dt {dt!r} or no data")
        vals = [float(v) for v in data.group(1).replace("\n", " ").split(",") if v.strip()]
        if len(vals) != rows * cols:
            raise ValueError(f"opencv-matrix {m.group(1)}: {len(vals)} values for {rows} x {cols}")
        out[m.group(1)] = np.array(vals, np.float64).reshape(rows, cols)
    for m in re.finditer(r"^(\w+):[ \t]*([-+0-9.eE]+)[ \t]*$", text, flags=re.M):
        out.setdefault(m.group(1), float(m.group(2)))
    return out


def load_calibration(path) -> Calibration:
    """calibration_parameters.npz (keys camera_matrix, dist_coeffs, image_size; the file's pickled object arrays are never
    touched: allow_pickle stays False) or calibration_parameters.yml (OpenCV FileStorage: image_width, image_height,
    camera_matrix, distortion_coefficients) -> Calibration.  4, 5, 8, 12 or 14 coefficients, zero-padded to 14."""
    path = Path(path)
    if path.suffix.lower() == ".npz":
        with np.load(str(path), allow_pickle=False) as z:
            missing = [k for k in ("camera_matrix", "dist_coeffs", "image_size") if k not in z.files]
            if missing:
                raise ValueError(f"{path}: no {missing[0]} entry")
            K, d, size = z["camera_matrix"], z["dist_coeffs"], z["image_size"]
    elif path.suffix.lower() in (".yml", ".yaml"):
        y = _opencv_yaml(path.read_text())
        try:
            K, d, size = y["camera_matrix"], y["distortion_coefficients"], (y["image_width"], y["image_height"])
        except KeyError as e:
            raise ValueError(f"{path}: no {e.args[0]} entry") from None
    else:
        raise ValueError(f"{path}: a calibration file is .npz or OpenCV .yml")
    K = np.array(K, dtype=np.float64)
    d = np.array(d, dtype=np.float64).reshape(-1)
    size = np.asarray(size).reshape(-1)
    if K.shape != (3, 3) or d.size not in (4, 5, 8, 12, 14) or size.size != 2:
        raise ValueError(f"{path}: camera_matrix {list(K.shape)}, {d.size} coefficients, image_size of {size.size} numbers")
    dist = np.zeros(14, np.float64)
    dist[:d.size] = d
    return Calibration(K, dist, (int(size[0]), int(size[1])))


def _opencv_matrix(name: str, a: np.ndarray) -> str:
    vals = [repr(float(v)) for v in a.reshape(-1)]
    lines, line = [], "   data: ["
    for k, v in enumerate(vals):
        piece = v + (", " if k + 1 < len(vals) else " ]")
        if len(line) + len(piece) > 76:
            lines.append(line.rstrip())
            line = "       "
        line += piece
    lines.append(line)
    return f"{name}: !!opencv-matrix\n   rows: {a.shape[0]}\n   cols: {a.shape[1]}\n   dt: d\n" + "\n".join(lines) + "\n"


def save_calibration(npz_path, yml_path, K, dist, image_size, rvecs=None, tvecs=None, used=(), used_full=None, dropped=(),
                     flags: int = 0) -> None:
    """What camera_calibration/main.py saves (:325-349) and `load_calibration` reads.  npz_path: camera_matrix [3, 3],
    dist_coeffs [1, k] (k = 4, 5, 8, 12 or 14), image_size (width, height), rvecs / tvecs [V, 3, 1], used, used_full,
    dropped as fixed-width string arrays -- no pickled object arrays, and no `config` entry (the reference pickles a dict).
    yml_path: OpenCV FileStorage with image_width, image_height, camera_matrix, distortion_coefficients, and flags.  Either
    path may be None.  Every float is written with repr, so both files read back to the same bits."""
    K = np.asarray(K, np.float64)
    d = np.asarray(dist, np.float64).reshape(-1)
    w, h = (int(x) for x in image_size)
    if K.shape != (3, 3) or d.size not in (4, 5, 8, 12, 14):
        raise ValueError(f"save_calibration: camera_matrix {list(K.shape)}, {d.size} coefficients (4, 5, 8, 12 or 14)")
    strs = lambda names: np.array([str(x) for x in names], dtype=np.str_).reshape(-1)      # noqa: E731
    if npz_path is not None:
        npz_path = Path(npz_path)
        npz_path.parent.mkdir(parents=True, exist_ok=True)
        vec = lambda a: np.zeros((0, 3, 1)) if a is None else np.asarray(a, np.float64).reshape(-1, 3, 1)     # noqa: E731
        np.savez(str(npz_path), camera_matrix=K, dist_coeffs=d[None], rvecs=vec(rvecs), tvecs=vec(tvecs),
                 image_size=np.array([w, h], np.int64), used=strs(used), used_full=strs(used if used_full is None else used_full),
                 dropped=strs(dropped))
    if yml_path is not None:
        yml_path = Path(yml_path)
        yml_path.parent.mkdir(parents=True, exist_ok=True)
        yml_path.write_text(f"%YAML:1.0\n---\nimage_width: {w}\nimage_height: {h}\n" + _opencv_matrix("camera_matrix", K)
                            + _opencv_matrix("distortion_coefficients", d[None]) + f"flags: {int(flags)}\n")
