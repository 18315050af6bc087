# one 148^2 x 32-frame 256 -> 256 slice-major conv launch of gemm_x3w4_kernel (after two warm-up launches), for
# separate rocprofv3 --pmc passes per MFMA shape:
#   SKIMI_X3_MFMA=16 rocprofv3 --kernel-trace --output-format csv --pmc SQ_LDS_BANK_CONFLICT -d DIR -- python tools/pmc_x3.py
import os, sys, math, torch
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from skiing_analysis_pytorch_amd import ops
from skiing_analysis_pytorch_amd._lib import PREC_BF16X3, ACT_RELU
D = "cuda"
n, H, W, C, N = 32, 148, 148, 256, 256
M, K = n * H * W, 9 * C
g = torch.Generator(device=D).manual_seed(0)
x = torch.randn(M, C, device=D, generator=g)
w = torch.randn(N, K, device=D, generator=g) / math.sqrt(K)
b = torch.randn(N, device=D, generator=g)
ar = ops.records_buffer(M, C)
nrec = M * (C // 32) * 64
ar[:nrec] = ops.split_records(x).reshape(-1)
ar[nrec:] = 0
ws, o = ops.split_records(w), torch.empty(M, N, device=D)
conv = dict(N=n, H=H, W=W, C=C, KH=3, KW=3, stride=1, pad=1, dil=1, OH=H, OW=W, slice_major=True)
for _ in range(3):
    ops.gemm(None, w, prec=PREC_BF16X3, conv=conv, bias=b, act=ACT_RELU, out=o, w_split=ws, a_records=ar)
torch.cuda.synchronize()
p = ops.gemm_last_path()
print(f"SKIMI_X3_MFMA={os.environ.get('SKIMI_X3_MFMA', '16')}: {p.family} mfma {p.mfma}", flush=True)
