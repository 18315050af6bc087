"""Call times of the device kinematic analysis next to the host restatement (and, where its tree is at hand, the
reference's own angle/main.py) on the same seeded skiers: B = 1, T = 243; B = 1, T = 1025; B = 32, T = 243.

    python tools/mb_kinematics.py [--reps 200] [--json out.json]

Device: HIP events around `reps` back-to-back calls after three warm-up calls, the median of five such rounds; once for
geometry.kinematics (the Python wrapper: twelve output allocations included) and once for skimi_kinematics alone on
preallocated buffers (the three launches).  Host: wall time per clip of tests/kinematics_restated.py (series, changes, turns
and statistics) and of the reference's _compute_all_series + compute_series_changes, the median of three."""
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

import kinematics_cases as kc  # noqa: E402
import kinematics_restated as kr  # noqa: E402
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


def raw_call(X):
    """skimi_kinematics on preallocated outputs -> a function that makes one call"""
    B, T, J = X.shape[:3]
    M = geometry.kin_max_turns(T)
    f64 = lambda *s: torch.empty(s, dtype=torch.float64, device="cuda")      # noqa: E731
    i32 = lambda *s: torch.empty(s, dtype=torch.int32, device="cuda")        # noqa: E731
    outs = [f64(B, 42, T), f64(B, T), f64(B, T), f64(B, T), torch.empty((B, T), dtype=torch.uint8, device="cuda"), i32(B),
            i32(B, M, 2), f64(B, M), i32(B, M), f64(B, M, 42, 4), i32(B, M, 42)]
    ptrs = [_lib.ptr(o) for o in outs]
    lay, up = (C.c_int32 * 13)(*kr.MHR70_15), (C.c_double * 3)(0.0, -1.0, 0.0)
    fn, st, xp = _lib.lib().skimi_kinematics, _lib.current_stream(), _lib.ptr(X)

    def call():
        _lib.check(fn(xp, None, B, T, J, lay, up, 12, 8.0, 11, 9, M, None, 0, *ptrs, st), "skimi_kinematics")

    call.keep = (X, outs)
    return call


def reference():
    ref = Path(os.environ.get("SKIMI_REFERENCE", "/root/reference")) / "angle" / "main.py"
    if not ref.exists():
        return None
    os.environ.setdefault("MPLBACKEND", "Agg")
    spec = importlib.util.spec_from_file_location("ref_angle_main", ref)
    A = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(A)
    return A


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--json", default=None)
    ap.add_argument("--host-only", action="store_true", help="the host columns alone (no device needed)")
    a = ap.parse_args()
    A = reference()
    rows = []
    for B, T in ((1, 243), (1, 1025), (32, 243)):
        X = np.stack([kc.skier(T, 900 + b) for b in range(B)])
        row = dict(B=B, T=T, restated_ms_per_clip=host_ms(lambda: kr.kinematics(X[0])))
        if A is not None:
            def ref_call():
                j, body, torso, kd, el, _, _ = A._compute_all_series(X[0], np.array([0.0, -1.0, 0.0]))
                A.compute_series_changes({**j, **torso, **kd, **el, **body})
            row["reference_ms_per_clip"] = host_ms(ref_call)
        if not a.host_only:
            Xd = torch.from_numpy(X).cuda()
            row["wrapper_ms"] = device_ms(lambda: geometry.kinematics(Xd), a.reps)
            row["library_ms"] = device_ms(raw_call(Xd), a.reps)
        rows.append(row)
    for r in rows:
        print("  ".join(f"{k} {v:.4f}" if isinstance(v, float) else f"{k} {v}" for k, v in r.items()))
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(rows, indent=1))


if __name__ == "__main__":
    main()
