"""Pass times of the scene-view renderer (csrc/scene_view.hip) beside a copy of the same clip and a torch formulation.

    python tools/mb_scene_view.py [--frames 243] [--reps 5] [--json out.json]      (on the GPU)
    python tools/mb_scene_view.py --resources                                      (registers and LDS; needs hipcc only)

The cloud is one VGGT step's worth of points, 8 x 518 x 518 = 2 146 592, on a rough surface with noise.  It is rendered (a)
into one 1080p frame and (b) into a `--frames`-frame 1080p orbit, in chunks of 16 frames (the default 256 MiB of key buffer).
skimi_scene_view_render runs memset + splat + resolve per chunk, so the passes are separated by leaving parts out, all
INTERLEAVED in one process:
    full       cloud, no primitives          memset + splat + resolve
    full_ps3   the same with point_size 3: nine keys a point (fewer at the frame's edges), neighbouring squares overlap
    no_cloud   no cloud, no primitives       memset + resolve            -> splat = full - no_cloud
    prims      no cloud, one skeleton and eight camera markers (121 records)   memset + resolve with primitives
    memset     torch's zero_() of the key buffer of one chunk, times the chunks
    clone      frames.clone() of the rendered clip: the store floor of the resolve pass
    torch      keys.scatter_reduce_(0, pixel, key, "amax") on the same keys (1 frame; the first 16-frame chunk of the orbit,
               scaled by frames / 16): the baseline to beat.  Building its keys with torch ops is NOT in the time.
HIP events around `reps` back-to-back calls after three warm-up calls; a round times every variant twice in turn; the figure is
the median of five rounds (min and max beside it).  The 64-bit atomic rate is (keys issued) / (splat time), keys issued = the
points that pass the fragment test and land in the frame, counted with the builders (geometry.view_project)."""
import argparse
import json
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from skiing_analysis_pytorch_amd import build as B, draw, geometry  # noqa: E402

H, W = 1080, 1920
CHUNK = 16


def resources():
    """the compiler's resource remarks for csrc/scene_view.hip under the build's flags -> rows"""
    cmd = [B.HIPCC, *B.CXXFLAGS, "-Rpass-analysis=kernel-resource-usage", "-c", str(B.CSRC / "scene_view.hip"), "-o", "/dev/null"]
    text = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    rows, cur = [], None
    for ln in text.splitlines():
        m = re.search(r"Function Name: \S*?(scene_\w+_kernel)", ln)
        if m:
            cur = dict(kernel=m.group(1))
            rows.append(cur)
        for key, pat in (("vgprs", r" VGPRs: (\d+)"), ("sgprs", r"TotalSGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("lds", r"LDS Size \[bytes/block\]: (\d+)"), ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)")):
            m = re.search(pat, ln)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    return rows


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def interleaved(fns, reps, rounds=5):
    """-> per function (median, min, max) ms over `rounds` rounds that time every function twice in turn"""
    for fn in fns:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(rounds):
        for _ in range(2):
            for k, fn in enumerate(fns):
                times[k].append(timed(fn, reps))
    return [(float(np.median(t)), float(min(t)), float(max(t))) for t in times]


def make_cloud(n, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    xy = torch.rand((n, 2), device="cuda", generator=g) * 2.0 - 1.0
    z = 0.25 * torch.sin(3.0 * xy[:, 0]) * torch.cos(2.0 * xy[:, 1]) + 0.02 * torch.randn(n, device="cuda", generator=g)
    xyz = torch.cat([xy, z[:, None]], dim=1).to(torch.float32).contiguous()[None]
    rgb = torch.randint(0, 256, (1, n, 3), dtype=torch.uint8, device="cuda", generator=g)
    return xyz, rgb


def keys_of(xyz, views):
    """the splat's keys with torch ops: (flat pixel int64 [m], key int64 [m]) of the points that land in their frame"""
    xy, w, ok = geometry.view_project(xyz[0], views)                       # [F, n, ...]
    fu, fv = torch.floor(xy[..., 0]), torch.floor(xy[..., 1])
    ok = ok & (fu >= 0) & (fu < W) & (fv >= 0) & (fv < H)
    f = torch.arange(views.shape[0], device="cuda")[:, None].expand_as(fu)
    pix = (f * (H * W) + fv.clamp(0, H - 1).long() * W + fu.clamp(0, W - 1).long())[ok]
    idx = torch.arange(xyz.shape[1], device="cuda")[None].expand_as(fu)
    return pix, ((w.long() << 32) | idx)[ok]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=243)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--resources", action="store_true")
    a = ap.parse_args()
    if a.resources:
        for row in resources():
            print(row)
        return
    n = 8 * 518 * 518
    xyz, rgb = make_cloud(n)
    centre = torch.zeros(3, dtype=torch.float64, device="cuda")
    rows = []
    for name, F in (("one_frame", 1), ("orbit", a.frames)):
        az = torch.arange(F, dtype=torch.float64, device="cuda") * (360.0 / F)
        views = geometry.orbit_view(centre, 3.0, 30.0, az, 0.8 * W, 0.8 * W, W / 2.0, H / 2.0, 0.1, 10.0).reshape(F, 20)
        # one skeleton and eight camera markers, built once
        joints = torch.from_numpy(np.random.default_rng(1).uniform(-0.3, 0.3, (17, 3)) + [0, 0, 0.6]).cuda()
        cam_views = geometry.orbit_view(centre, 1.5, 20.0, torch.arange(8, dtype=torch.float64, device="cuda") * 45.0, 500.0, 500.0, 320.0, 240.0, 0.1, 10.0)
        E = cam_views[:, :12].reshape(8, 3, 4)
        K = torch.tensor([[500.0, 0, 320.0], [0, 500.0, 240.0], [0, 0, 1.0]], dtype=torch.float64, device="cuda").expand(8, 3, 3)
        prims = geometry.cat_prims(geometry.skeleton_prims(joints, draw.COCO_SKELETON, views), geometry.camera_prims(E, K, views, 0.1, 0.15))
        out = torch.empty((F, H, W, 3), dtype=torch.uint8, device="cuda")
        chunks = -(-F // CHUNK)
        keybuf = torch.empty((min(F, CHUNK) * H * W,), dtype=torch.int64, device="cuda")
        Fb = min(F, CHUNK)
        pix, key = keys_of(xyz, views[:Fb])
        issued_b = int(key.numel())
        issued = issued_b if F <= CHUNK else sum(int(keys_of(xyz, views[c:c + CHUNK])[1].numel()) for c in range(0, F, CHUNK))
        base = torch.zeros((Fb * H * W,), dtype=torch.int64, device="cuda")

        def torch_splat():
            base.zero_()
            base.scatter_reduce_(0, pix, key, "amax", include_self=True)

        def memset():
            for _ in range(chunks):
                keybuf.zero_()

        fns = (lambda: geometry.render_scene(views, xyz, rgb, size=(H, W), out=out),
               lambda: geometry.render_scene(views, xyz, rgb, point_size=3, size=(H, W), out=out),
               lambda: geometry.render_scene(views, size=(H, W), out=out),
               lambda: geometry.render_scene(views, prims=prims, size=(H, W), out=out),
               memset, lambda: out.clone(), torch_splat)
        (full, full3, no_cloud, with_prims, ms, clone, tsp) = interleaved(fns, a.reps)
        # the torch formulation gives the kernel's keys
        got = geometry.render_scene(views[:Fb], xyz, rgb, size=(H, W), want_index=True)
        torch_splat()
        same = bool(torch.equal(torch.where(base > 0, base & 0xFFFFFFFF, torch.full_like(base, -1)).to(torch.int32).reshape(Fb, H, W), got.index))
        splat_ms = full[0] - no_cloud[0]
        scale = F / Fb
        rows.append(dict(case=name, frames=F, points=n, chunks=chunks, records_per_frame=int(prims.shape[-2]), keys_issued=issued,
                         full_ms=full[0], full_ms_min=full[1], full_ms_max=full[2], no_cloud_ms=no_cloud[0], no_cloud_ms_min=no_cloud[1],
                         no_cloud_ms_max=no_cloud[2], prims_ms=with_prims[0], prims_ms_min=with_prims[1], prims_ms_max=with_prims[2],
                         memset_ms=ms[0], clone_ms=clone[0], clone_ms_min=clone[1], clone_ms_max=clone[2],
                         full_ps3_ms=full3[0], full_ps3_ms_min=full3[1], full_ps3_ms_max=full3[2], splat_ps3_ms=full3[0] - no_cloud[0],
                         atomic_keys_per_s_ps3_upper=9 * issued / ((full3[0] - no_cloud[0]) * 1e-3),
                         splat_ms=splat_ms, threads_per_s=F * n / (splat_ms * 1e-3), atomic_keys_per_s=issued / (splat_ms * 1e-3),
                         resolve_ms=no_cloud[0] - ms[0], resolve_prims_ms=with_prims[0] - ms[0], resolve_over_clone=(no_cloud[0] - ms[0]) / clone[0],
                         resolve_prims_over_clone=(with_prims[0] - ms[0]) / clone[0],
                         torch_scatter_frames=Fb, torch_scatter_ms=tsp[0], torch_scatter_ms_min=tsp[1], torch_scatter_ms_max=tsp[2],
                         torch_scatter_scaled_ms=tsp[0] * scale, torch_keys_per_s=issued_b / (tsp[0] * 1e-3), torch_equals_kernel=same,
                         splat_over_torch=splat_ms / (tsp[0] * scale)))
    for row in rows:
        print("  ".join(f"{k} {v:.4f}" if isinstance(v, float) else f"{k} {v}" for k, v in row.items()), flush=True)
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(dict(rows=rows), indent=1))


if __name__ == "__main__":
    main()
