# interleaved A/B timing, in one process, of the launches that SKIMI_DPT_OC1_COARSE replaces in a bf16x3 DPT head at the
# bench's shapes (32 frames, refinenet1's 148 x 148 map of 256 features, output_conv1 256 -> 128 on 296 x 296)
#   fine   : out_conv (records in, fp32 rows out) + bilinear_ac_planes (x2, into records) + the 3x3 conv as a slice-major
#            gather GEMM on the 128-column LDS-DMA kernel -- what run_dpt launches with SKIMI_DPT_OC1_COARSE=0
#   coarse : out_conv (records in, records out) + the nine taps' contraction, one plain-row GEMM of N = 1152 on the
#            256-column LDS-DMA kernel (4.5 column tiles) + dpt_tap_sum
#   coarse9: the same with the contraction as nine launches of 128 columns on the 128-column kernel
# every part is also timed alone.    python tools/ab_dpt_oc1.py            (AB_REPS: rounds, default 5)
import os, sys, math, torch
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from skiing_analysis_pytorch_amd import ops
from skiing_analysis_pytorch_amd._lib import PREC_BF16X3
from tools.microbench import timeit
D = "cuda"
Fr, h, w, C, Co = int(os.environ.get("AB_FRAMES", 32)), 148, 148, 256, 128
H, W = 2 * h, 2 * w
M0, M1 = Fr * h * w, Fr * H * W
g = torch.Generator(device=D).manual_seed(0)
u = torch.randn(M0, C, device=D, generator=g)
w_oc = torch.randn(C, C, device=D, generator=g) / math.sqrt(C)
b_oc = torch.randn(C, device=D, generator=g)
w1 = torch.randn(Co, C, 3, 3, device=D, generator=g) / math.sqrt(9 * C)
b1 = torch.randn(Co, device=D, generator=g)
u_rec = ops.records_buffer(M0, C)
u_rec[:M0 * C * 2] = ops.split_records(u).reshape(-1)
u_rec[M0 * C * 2:] = 0
del u
w_oc_s = ops.split_records(w_oc)
# fine
olow = torch.empty(Fr, h, w, C, device=D)
rec = ops.records_buffer(M1, C)
wsl = w1.permute(0, 2, 3, 1).reshape(Co, 3, 3, C // 32, 32).permute(0, 3, 1, 2, 4).reshape(Co, 9 * C).contiguous()
wsl_s = ops.split_records(wsl)
conv = dict(N=Fr, H=H, W=W, C=C, KH=3, KW=3, stride=1, pad=1, dil=1, OH=H, OW=W, slice_major=True)
o_fine = torch.empty(M1, Co, device=D)
# coarse
orec = ops.records_buffer(M0, C)
w9 = ops.conv3x3_taps_matrix(w1)
w9_s = ops.split_records(w9)
w9_t = [w9[t * Co:(t + 1) * Co] for t in range(9)]
w9_ts = [ops.split_records(x.contiguous()) for x in w9_t]
taps = torch.empty(M0, 9 * Co, device=D)
o_coarse = torch.empty(Fr, H, W, Co, device=D)


def out_conv_rows():
    ops.gemm(None, w_oc, prec=PREC_BF16X3, bias=b_oc, a_records=u_rec, M=M0, lda=C, w_split=w_oc_s, out=olow.view(M0, C))


def upsample():
    ops.resize_bilinear_planes(olow, H, W, rec, records=True, zpage=rec[M1 * C * 2:])


def conv3x3():
    ops.gemm(None, wsl, prec=PREC_BF16X3, conv=conv, bias=b1, a_records=rec, w_split=wsl_s, out=o_fine)


def out_conv_records():
    ops.gemm(None, w_oc, prec=PREC_BF16X3, bias=b_oc, a_records=u_rec, M=M0, lda=C, w_split=w_oc_s, out_records=orec, records_only=True)


def contract_wide():
    ops.gemm(None, w9, prec=PREC_BF16X3, a_records=orec, M=M0, lda=C, w_split=w9_s, out=taps)


def contract_nine():
    for t in range(9):
        ops.gemm(None, w9_t[t], prec=PREC_BF16X3, a_records=orec, M=M0, lda=C, w_split=w9_ts[t], out=taps[:, t * Co:(t + 1) * Co])


def tap_sum():
    ops.dpt_tap_sum(taps.view(Fr, h, w, 9, Co), b1, out=o_coarse)


def fine():
    out_conv_rows(); upsample(); conv3x3()


def coarse():
    out_conv_records(); contract_wide(); tap_sum()


def coarse9():
    out_conv_records(); contract_nine(); tap_sum()


fine()
print("fine conv on:", ops.gemm_last_path().family, flush=True)
out_conv_records(); contract_nine()
t9 = taps.clone()
contract_wide()
print("contraction on:", ops.gemm_last_path().family, " nine launches == one launch:", bool(torch.equal(t9, taps)), flush=True)
del t9
tap_sum()
torch.cuda.synchronize()
d = (o_coarse.view(M1, Co) - o_fine).abs().max().item() / o_fine.abs().max().item()
print(f"coarse vs fine: max abs difference / max abs value {d:.2e}", flush=True)
fns = dict(fine=fine, coarse=coarse, coarse9=coarse9, out_conv_rows=out_conv_rows, upsample=upsample, conv3x3=conv3x3,
           out_conv_records=out_conv_records, contract_wide=contract_wide, contract_nine=contract_nine, tap_sum=tap_sum)
res = {k: [] for k in fns}
for rep in range(int(os.environ.get("AB_REPS", 5))):
    for k in fns:
        res[k].append(timeit(fns[k], iters=10, warm=2))
med = {}
for k in fns:
    ts = sorted(res[k])
    med[k] = ts[len(ts) // 2]
    print(f"{k:17s}: median {med[k] * 1e6:8.1f} us  (min {ts[0] * 1e6:.1f})", flush=True)
gb = (M0 * 9 * Co * 4 + M1 * Co * 4) / 1e9
print(f"tap_sum moves {gb:.2f} GB (T once + out): {gb / med['tap_sum'] / 1e3:.2f} TB/s", flush=True)
print(f"fine -> coarse : {100 * (med['coarse'] / med['fine'] - 1):+.1f} %", flush=True)
print(f"fine -> coarse9: {100 * (med['coarse9'] / med['fine'] - 1):+.1f} %", flush=True)
