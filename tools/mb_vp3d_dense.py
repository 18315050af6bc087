"""TemporalModel(dense=True) timing (profiles/vp3d_dense.md), RF 27 (269 -> 243 frames) and RF 243 (485 -> 243).

    python tools/mb_vp3d_dense.py              # time per clip (HIP events) at B = 1, 2, 64; window vs per-tap kernel
                                               # interleaved in one process; torch fp32 conv1d at the wide convs' shapes
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/mb_vp3d_dense.py --trace
    python tools/mb_vp3d_dense.py --layers DIR # per-layer kernel times of that trace, against their bounds

The A/B flips SKIMI_VP3D_WINDOW between 1 and 0 inside one process (SKIMI_ENV_DYNAMIC=1: the switch is re-read on every
forward).  The bound of a result is the larger of 3 x its FLOPs (bf16x3: three bf16 products per product) over the
LDS-fed v_mfma_f32_16x16x32_bf16 rate of profiles/r04_peaks.json (1853 TFLOP/s), and its record bytes (weights,
inputs and outputs as hi + lo bf16 pairs, 4 B per element) over 6.3 TB/s.
"""
import csv
import glob
import os
import statistics
import sys
from pathlib import Path

os.environ.setdefault("SKIMI_ENV_DYNAMIC", "1")

import torch  # noqa: E402

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

MFMA_RATE, HBM = 1853e12, 6.3e12
C = 1024
CASES = (([3, 3, 3], 269), ([3, 3, 3, 3, 3], 485))
TRACE_B, TRACE_REPS = (1, 2), 6


def layers(fw, lin, B):
    """[(name, taps, Lin, Lout, N, K, FLOPs, record bytes)] of one forward, in launch order"""
    pad, nd = [fw[0] // 2], fw[0]
    for w in fw[1:]:
        pad.append((w - 1) * nd // 2)
        nd *= w
    L = lin - fw[0] + 1
    out = [("expand", fw[0], lin, L, C, fw[0] * 34)]
    for i in range(1, len(fw)):
        t = 2 * pad[i] + 1
        out.append((f"block {i} conv", t, L, L - t + 1, C, t * C))
        L = L - t + 1
        out.append((f"block {i} 1x1", 1, L, L, C, C))
    out.append(("shrink", 1, L, L, 51, C))
    return [(n, t, li, lo, N, K, 2.0 * B * lo * N * K, 4.0 * (N * K + B * li * K / t + B * lo * N)) for n, t, li, lo, N, K in out]


def bound(flops, nbytes):
    a, b = 3 * flops / MFMA_RATE, nbytes / HBM
    return (a, "MFMA") if a >= b else (b, "bytes")


def model(fw):
    from skiing_analysis_pytorch_amd import vp3d, weights as W
    from skiing_analysis_pytorch_amd._lib import PREC_BF16X3

    m = vp3d.TemporalModel(17, 2, 17, fw, dense=True, prec=PREC_BF16X3)
    m.load_state_dict(W.make_vp3d_state_dict(seed=0, filter_widths=fw, dense=True))
    return m


def main():
    from tools.microbench import timeit

    print(torch.cuda.get_device_name(0))
    for fw, lin in CASES:
        m = model(fw)
        rf = m.receptive_field()
        print(f"\n## RF {rf} dense ({lin} -> 243 frames)")
        print("| B | path | us / call | us / clip | bound (us / call, kind) | share of bound |\n|---|---|---:|---:|---:|---:|")
        for B in (1, 2, 64):
            x = torch.randn(B, lin, 17, 2, device="cuda")
            out = torch.empty(B, 243, 17, 3, device="cuda")
            ls = layers(fw, lin, B)
            b, kind = bound(sum(r[6] for r in ls), sum(r[7] for r in ls))
            t = timeit(lambda: m(x, out=out), iters=10 if B == 64 else 30, warm=3)
            path = "GEMM chain" if B * (lin - 2) > 2048 else "streaming"
            print(f"| {B} | {path} | {t * 1e6:.1f} | {t * 1e6 / B:.1f} | {b * 1e6:.1f} ({kind}) | {b / t * 100:.1f} % |", flush=True)
        # interleaved A/B: window kernel (1) vs per-tap kernel (0), same process, same buffers
        print("\n| B | window us / call | per-tap us / call | per-tap / window |\n|---|---:|---:|---:|")
        for B in (1, 2):
            x = torch.randn(B, lin, 17, 2, device="cuda")
            out = torch.empty(B, 243, 17, 3, device="cuda")
            ts = {"1": [], "0": []}
            for _ in range(5):
                for v in ("1", "0"):
                    os.environ["SKIMI_VP3D_WINDOW"] = v
                    ts[v].append(timeit(lambda: m(x, out=out), iters=10, warm=2))
            os.environ["SKIMI_VP3D_WINDOW"] = "1"
            w, p = statistics.median(ts["1"]), statistics.median(ts["0"])
            print(f"| {B} | {w * 1e6:.1f} | {p * 1e6:.1f} | {p / w:.2f} |", flush=True)
        del m
        torch.cuda.empty_cache()
    # yardstick: torch fp32 conv1d (timed only; the product never calls it) at the wide convs' shapes, B = 2
    print("\n| torch fp32 conv1d, B = 2 | us |\n|---|---:|")
    for fw, lin in CASES:
        for n, t, li, lo, N, K, fl, nb in layers(fw, lin, 2):
            if t > 1 and n != "expand":
                x = torch.randn(2, C, li, device="cuda")
                w = torch.randn(C, C, t, device="cuda") / (C * t) ** 0.5
                tt = timeit(lambda: torch.nn.functional.conv1d(x, w), iters=10, warm=2)
                print(f"| RF {lin - 242} {n} ({t} taps) | {tt * 1e6:.1f} |", flush=True)


def trace():
    """The schedule --layers expects: per case, per B, per variant (window, per-tap): TRACE_REPS forwards."""
    for fw, lin in CASES:
        m = model(fw)
        for B in TRACE_B:
            x = torch.randn(B, lin, 17, 2, device="cuda")
            out = torch.empty(B, 243, 17, 3, device="cuda")
            for v in ("1", "0"):
                os.environ["SKIMI_VP3D_WINDOW"] = v
                for _ in range(TRACE_REPS):
                    m(x, out=out)
                torch.cuda.synchronize()
        del m
        torch.cuda.empty_cache()
    print("trace done")


def per_layer(d):
    paths = sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True))
    assert paths, f"no kernel_trace.csv under {d}"
    rows = []
    for p in paths:
        rows += [r for r in csv.DictReader(open(p)) if "vp3d_" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    i = 0
    for fw, lin in CASES:
        for B in TRACE_B:
            ls = layers(fw, lin, B)
            res = {}
            for v in ("1", "0"):
                per = [[] for _ in ls]
                for _ in range(TRACE_REPS):
                    for j in range(len(ls)):
                        r = rows[i]
                        i += 1
                        per[j].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-9)
                        if _ == TRACE_REPS - 1:
                            per[j].append(r["Kernel_Name"].split("(")[0].replace("void ", "").replace("skimi::", ""))
                res[v] = [(statistics.median(p[1:-1]), p[-1]) for p in per]   # first forward: warm-up
            print(f"\n### RF {lin - 242} dense, B = {B}\n")
            print("| layer | taps | window kernel us | share of bound | per-tap us | per-tap / window | bound us (kind) |")
            print("|---|---:|---:|---:|---:|---:|---:|")
            for (n, t, li, lo, N, K, fl, nb), (tw, kw), (tp, kp) in zip(ls, res["1"], res["0"]):
                b, kind = bound(fl, nb)
                print(f"| {n} | {t} | {tw * 1e6:.1f} | {b / tw * 100:.1f} % | {tp * 1e6:.1f} | {tp / tw:.2f} | {b * 1e6:.1f} ({kind}) |"
                      + (f" <!-- {kw} / {kp} -->" if kw != kp else ""))
    assert i == len(rows), (i, len(rows))


if __name__ == "__main__":
    if "--trace" in sys.argv:
        trace()
    elif "--layers" in sys.argv:
        per_layer(sys.argv[sys.argv.index("--layers") + 1])
    else:
        main()
