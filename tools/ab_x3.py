# interleaved A/B timing of the bf16x3 DPT-head kernels (gemm_x3dma.hip) on both MFMA shapes inside one process
# (SKIMI_ENV_DYNAMIC=1, SKIMI_X3_MFMA = 32 | 16), at the bench's shapes (32 frames), operands as pre-split records:
#   python tools/ab_x3.py            (AB_REPS: rounds over all shapes, default 5; AB_ONLY=name[,name]: a subset)
import os, sys, math, torch
os.environ["SKIMI_ENV_DYNAMIC"] = "1"
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from skiing_analysis_pytorch_amd import ops
from skiing_analysis_pytorch_amd._lib import PREC_BF16X3, ACT_RELU
from tools.microbench import timeit
D = "cuda"
SHAPES = {  # name -> (rows of the A image, C, N, conv geometry or None: plain rows)
    "conv148": (32 * 148 * 148, 256, 256, (148, 148)),
    "conv74": (32 * 74 * 74, 256, 256, (74, 74)),
    "conv37": (32 * 37 * 37, 256, 256, (37, 37)),
    "proj256": (43808, 2048, 256, None),
    "proj512": (43808, 2048, 512, None),
    "proj1024": (43808, 2048, 1024, None),
    "conv296n": (32 * 296 * 296, 256, 128, (296, 296)),
}
only = os.environ.get("AB_ONLY")
names = [n for n in SHAPES if not only or n in only.split(",")]
g = torch.Generator(device=D).manual_seed(0)


def records(x):
    ar = ops.records_buffer(*x.shape)
    nrec = x.shape[0] * ((x.shape[1] + 31) // 32) * 64
    ar[:nrec] = ops.split_records(x).reshape(-1)
    ar[nrec:] = 0
    return ar


fns, flops = {}, {}
for name in names:
    rows, C, N, hw = SHAPES[name]
    K = C * (9 if hw else 1)
    x = torch.randn(rows, C, device=D, generator=g)
    ar = records(x)
    del x
    w = torch.randn(N, K, device=D, generator=g) / math.sqrt(K)
    ws = ops.split_records(w)
    b = torch.randn(N, device=D, generator=g)
    o = torch.empty(rows, N, device=D)
    if hw:
        conv = dict(N=32, H=hw[0], W=hw[1], C=C, KH=3, KW=3, stride=1, pad=1, dil=1, OH=hw[0], OW=hw[1], slice_major=True)
        fns[name] = lambda ar=ar, w=w, ws=ws, b=b, o=o, conv=conv: ops.gemm(None, w, prec=PREC_BF16X3, conv=conv, bias=b, act=ACT_RELU,
                                                                            out=o, w_split=ws, a_records=ar)
    else:
        fns[name] = lambda ar=ar, w=w, ws=ws, b=b, o=o, rows=rows, K=K: ops.gemm(None, w, prec=PREC_BF16X3, bias=b, out=o, w_split=ws,
                                                                                 a_records=ar, M=rows, lda=K)
    flops[name] = 2.0 * rows * N * K
variants = ["32", "16"]
res = {(v, n): [] for v in variants for n in names}
for rep in range(int(os.environ.get("AB_REPS", 5))):
    for n in names:
        for v in variants:
            os.environ["SKIMI_X3_MFMA"] = v
            fns[n]()
            p = ops.gemm_last_path()
            assert p.family.startswith("x3dma") and p.mfma == int(v), (n, v, p)
            res[(v, n)].append(timeit(fns[n], iters=10, warm=2))
for n in names:
    med = {}
    for v in variants:
        ts = sorted(res[(v, n)])
        med[v] = ts[len(ts) // 2]
        print(f"{n:9s} MFMA={v}: median {med[v] * 1e6:8.1f} us  {3 * flops[n] / med[v] / 1e12:6.0f} TF/s of MFMA work  (min {ts[0] * 1e6:.1f})",
              flush=True)
    print(f"{n:9s} 32 -> 16: {100 * (med['16'] / med['32'] - 1):+.1f} %", flush=True)
