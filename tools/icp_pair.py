"""Cost of the multi-view ICP step (cfg.infer.icp) on one pair of 518 x 518 world-point maps from VGGT-1B
(random-init weights, the bench scene's first two views): wall time, iterations, the normals / grid stages and
one iteration, against the VGGT call of that time step and the float64 restatement on the host.

    python tools/icp_pair.py [--out result.json] [--no-cpu]

One JSON object is printed (and written with --out); profiles/icp_pair.md records a run.
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def wall(fn, reps=3):
    """median host wall time of fn() (the ICP entry points synchronise their stream)"""
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-cpu", action="store_true", help="skip the host restatement (profiling runs)")
    ap.add_argument("--cpu-iters", type=int, default=5, help="iterations of the host restatement that are timed")
    args = ap.parse_args()

    from skiing_analysis_pytorch_amd import geometry, vggt, weights as W
    from skiing_analysis_pytorch_amd._lib import PREC_BF16X3, PREC_F16

    dev = torch.device("cuda", 0)
    cfg = W.VGGTConfig()
    model = vggt.VGGT(config=cfg, prec=PREC_F16, head_prec=PREC_BF16X3)
    model.load_state_dict(W.make_vggt_state_dict(cfg, seed=0, device=dev))
    g = torch.Generator(device=dev).manual_seed(1234)       # bench.py's scene: the first two views of its first step
    images = torch.rand((1, 8, 3, 518, 518), generator=g, device=dev, dtype=torch.float32)[:, :2].contiguous()

    def vggt_call():
        with torch.no_grad():
            out = model(images, want={"camera", "depth"})
            E, K = geometry.pose_encoding_to_extri_intri(out["pose_enc"], (518, 518))
            return geometry.unproject_depth_map_to_point_map(out["depth"][0], E[0], K[0])

    wp = vggt_call()
    t_vggt = wall(vggt_call)
    src, tgt = wp[0].reshape(-1, 3).contiguous(), wp[1].reshape(-1, 3).contiguous()

    res = geometry.icp_point_to_plane(src, tgt)
    t_full = wall(lambda: geometry.icp_point_to_plane(src, tgt))
    t_eval0 = wall(lambda: geometry.icp_point_to_plane(src, tgt, max_iteration=0))   # filter + grid + normals + 1 evaluation
    t_normals = wall(lambda: geometry.estimate_normals(tgt, 0.05))                      # filter + grid + normals
    t_corr = wall(lambda: geometry.icp_correspondences(src, tgt, np.eye(4), 0.05))     # filter of both + grid + 1 search
    normals, counts = geometry.estimate_normals(tgt, 0.05)
    c = counts.cpu().numpy()
    tn = tgt.cpu().numpy()
    extent = np.percentile(tn[np.isfinite(tn).all(1)], [1, 50, 99], axis=0).tolist()
    r = {
        "pair": "VGGT-1B (random-init weights, seed 0) on the bench scene's views 0 and 1, 518 x 518 -> 268 324 points per map",
        "vggt_call_s": t_vggt,
        "icp_wall_s": t_full,
        "icp_iterations": res.iterations,
        "icp_fitness": res.fitness,
        "icp_inlier_rmse": res.inlier_rmse,
        "icp_transformation": res.transformation.tolist(),
        "icp_max_iteration_0_s": t_eval0,
        "per_iteration_s": (t_full - t_eval0) / max(res.iterations, 1),
        "estimate_normals_s": t_normals,
        "correspondences_one_pass_s": t_corr,
        "neighbours_per_ball": {"median": float(np.median(c)), "p99": float(np.percentile(c, 99)), "max": int(c.max())},
        "target_extent_p1_p50_p99": extent,
    }
    if not args.no_cpu:
        import icp_restated as ref

        s_np, t_np = src.cpu().numpy(), tgt.cpu().numpy()
        t0 = time.perf_counter()
        P = t_np[ref.valid_mask(t_np)]
        ref.normals(P, 0.05)
        t_cpu_normals = time.perf_counter() - t0
        t0 = time.perf_counter()
        _, _, _, it = ref.icp_point_to_plane(s_np, t_np, max_iteration=args.cpu_iters)
        t_cpu = time.perf_counter() - t0
        per_it = (t_cpu - t_cpu_normals) / (it + 1)
        r["cpu_restatement"] = {"normals_s": t_cpu_normals, f"icp_{it}_iterations_s": t_cpu, "per_evaluation_s": per_it,
                                "estimated_full_s": t_cpu_normals + per_it * (res.iterations + 1)}
    line = json.dumps(r)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
