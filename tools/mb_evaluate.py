"""Call times of the device pose evaluation next to the host restatement (and, where its tree is at hand, the reference's
own functions) on the same seeded clips at J = 17: B = 1, T = 243; B = 1, T = 1025; B = 32, T = 243.

    python tools/mb_evaluate.py [--reps 200] [--json out.json] [--host-only]

Device: HIP events around `reps` back-to-back calls after three warm-up calls, the median of five such rounds; once for the
wrappers (geometry.pose_errors: its output allocations included; geometry.clip_quality) and once for skimi_pose_errors (three
launches) and skimi_clip_quality (one launch) alone on preallocated buffers.  Host, wall time per clip, the median of three:
tests/evaluate_restated.py, and the reference's loss.py (mpjpe, p_mpjpe, n_mpjpe, mean_velocity_error) + the per-frame
calculate_per_joint_errors loop with summarize_joint_errors for the errors, fuse_eval.py's bone_lengths + temporal_stats +
symmetry_score_mirror for the quality.  Also prints the worst device - restatement difference per output on these clips."""
import argparse
import ctypes as C
import importlib.util
import json
import os
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tests"))

import evaluate_cases as ec  # noqa: E402
import evaluate_restated as er  # noqa: E402
from skiing_analysis_pytorch_amd import _lib, geometry  # noqa: E402


def device_ms(fn, reps):
    for _ in range(3):
        fn()
    rounds = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        rounds.append(a.elapsed_time(b) / reps)
    return float(np.median(rounds))


def host_ms(fn):
    times = []
    for _ in range(3):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times))


def raw_pose_errors(P, G):
    B, T, J = P.shape[:3]
    f64 = lambda *s: torch.empty(s, dtype=torch.float64, device="cuda")      # noqa: E731
    i32 = lambda *s: torch.empty(s, dtype=torch.int32, device="cuda")        # noqa: E731
    outs = [f64(B, T, J), f64(B, T, J), f64(B, T, J), f64(B, T), f64(B, T), f64(B, T), i32(B, T), i32(B, T), None, None, None, None,
            f64(B, 4), i32(B, 3), f64(B, 2, J, 3), i32(B, 2, J)]
    ptrs = [_lib.ptr(o) for o in outs]
    fn, st, pp, gp = _lib.lib().skimi_pose_errors, _lib.current_stream(), _lib.ptr(P), _lib.ptr(G)

    def call():
        _lib.check(fn(pp, gp, None, B, T, J, -1, *ptrs, st), "skimi_pose_errors")

    call.keep = (P, G, outs)
    return call


def raw_clip_quality(X):
    B, T, J = X.shape[:3]
    lists = [np.asarray(v, dtype=np.int32).reshape(-1) for v in (er.H36M_EDGES, er.H36M_LEFT_BONES, er.H36M_RIGHT_BONES, er.H36M_LR_PAIRS)]
    c = [(C.c_int32 * v.size)(*v.tolist()) for v in lists]
    nbytes = int(_lib.lib().skimi_eval_workspace_bytes(B, T, J)) if T * J > geometry.EVAL_LDS_ELEMS else 0
    ws = torch.empty(max(nbytes, 8) // 8, dtype=torch.float64, device="cuda") if nbytes else None
    outs = [torch.empty(s, dtype=torch.float64, device="cuda") for s in ((B, 8), (B, 16), (B, T, 16))]
    fn, st, xp = _lib.lib().skimi_clip_quality, _lib.current_stream(), _lib.ptr(X)

    def call():
        _lib.check(fn(xp, None, B, T, J, c[0], 16, c[1], 6, c[2], 6, c[3], 6, _lib.ptr(ws), nbytes, *[_lib.ptr(o) for o in outs], st),
                   "skimi_clip_quality")

    call.keep = (X, ws, outs)
    return call


def reference():
    root = Path(os.environ.get("SKIMI_REFERENCE", "/root/reference"))
    if not (root / "VideoPose3D" / "common" / "loss.py").exists():
        return None

    def load(name, *parts):
        spec = importlib.util.spec_from_file_location(name, root.joinpath(*parts))
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
        return m

    return (load("ref_loss", "VideoPose3D", "common", "loss.py"), load("ref_fuse_eval", "VideoPose3D", "fuse", "fuse_eval.py"),
            load("ref_unity_data_compare", "metrics", "unity_data_compare.py"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--json", default=None)
    ap.add_argument("--host-only", action="store_true", help="the host columns alone (no device needed)")
    a = ap.parse_args()
    ref = reference()
    rows, worst = [], {}
    lay = ec.layout(17)
    for B, T in ((1, 243), (1, 1025), (32, 243)):
        clips = [ec.pose_clip(T, 17, 900 + b) for b in range(B)]
        P, G = np.stack([c[0] for c in clips]), np.stack([c[1] for c in clips])
        row = dict(B=B, T=T, restated_errors_ms_per_clip=host_ms(lambda: er.pose_errors(P[0], G[0])),
                   restated_quality_ms_per_clip=host_ms(lambda: er.clip_quality(P[0], **lay)))
        if ref is not None:
            loss, fe, udc = ref
            p, g = P[0], G[0]

            def ref_errors():
                loss.mpjpe(torch.from_numpy(p), torch.from_numpy(g))
                loss.n_mpjpe(torch.from_numpy(p)[None], torch.from_numpy(g)[None])
                loss.p_mpjpe(p.copy(), g.copy())
                loss.mean_velocity_error(p, g)
                box = udc.init_joint_stat_container(range(17))
                for t in range(T):
                    udc.accumulate_joint_errors(box, udc.calculate_per_joint_errors(dict(enumerate(p[t])), dict(enumerate(g[t]))))
                udc.summarize_joint_errors(box)

            def ref_quality():
                fe.eval_fused_pose(p, g, p)

            row["reference_errors_ms_per_clip"] = host_ms(ref_errors)
            row["reference_eval_fused_pose_ms_per_clip"] = host_ms(ref_quality)
        if not a.host_only:
            Pd, Gd = torch.from_numpy(P).cuda(), torch.from_numpy(G).cuda()
            row["pose_errors_wrapper_ms"] = device_ms(lambda: geometry.pose_errors(Pd, Gd), a.reps)
            row["pose_errors_library_ms"] = device_ms(raw_pose_errors(Pd, Gd), a.reps)
            row["clip_quality_wrapper_ms"] = device_ms(lambda: geometry.clip_quality(Pd), a.reps)
            row["clip_quality_library_ms"] = device_ms(raw_clip_quality(Pd), a.reps)
            r, q = geometry.pose_errors(Pd, Gd, aligned=True), geometry.clip_quality(Pd)
            wp, wq = er.pose_errors(P, G), er.clip_quality(P, **lay)
            for k in er.PE_FRAME_FLOATS + er.PE_CLIP_FLOATS:
                worst[k] = max(worst.get(k, 0.0), er.worst(getattr(r, k).cpu().numpy(), wp[k]))
            for k in er.CQ_FLOATS:
                worst[k] = max(worst.get(k, 0.0), er.worst(getattr(q, k).cpu().numpy(), wq[k]))
        rows.append(row)
    for r in rows:
        print("  ".join(f"{k} {v:.4f}" if isinstance(v, float) else f"{k} {v}" for k, v in r.items()))
    if worst:
        print("worst |device - restatement| / (1 + |x|): " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(dict(rows=rows, worst=worst), indent=1))


if __name__ == "__main__":
    main()
