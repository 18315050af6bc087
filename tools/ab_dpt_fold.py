# interleaved A/B timing, in one process, of the launches that SKIMI_DPT_FOLD replaces in a bf16x3 DPT head at the bench's
# shapes (32 frames of 37 x 37 patches): levels 0 (256 ch, stride 4) and 1 (512 ch, stride 2)
#   unfolded : ConvTranspose as a pixel-shuffle GEMM (fp32 A, split pass included) + layer_rn 3x3 conv (fp32 A, split pass
#              included, fp32 rows + records out, ReLU) -- what run_dpt launches with SKIMI_DPT_FOLD=0
#   folded   : ONE launch of s x s phase convs on the coarse map (A records in, fp32 rows + records out, ReLU)
# (the UV-embedding pass that precedes both is not timed: it reads and writes the same bytes either way)
#   python tools/ab_dpt_fold.py            (AB_REPS: rounds, default 5)
import os, sys, math, torch
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from skiing_analysis_pytorch_amd import ops
from skiing_analysis_pytorch_amd._lib import PREC_BF16X3, ACT_RELU
from tools.microbench import timeit
D = "cuda"
Fr, h, w, Co = 32, 37, 37, 256
g = torch.Generator(device=D).manual_seed(0)
fns, flops = {}, {}
for lvl, (C, s) in enumerate([(256, 4), (512, 2)]):
    x = torch.randn(Fr, h, w, C, device=D, generator=g)
    wT = torch.randn(C, C, s, s, device=D, generator=g) / math.sqrt(C)
    bT = torch.randn(C, device=D, generator=g)
    wrn = torch.randn(Co, C, 3, 3, device=D, generator=g) / math.sqrt(9 * C)
    M0, M1 = Fr * h * w, Fr * h * s * w * s
    # unfolded
    wps = wT.permute(2, 3, 1, 0).reshape(s * s * C, C).contiguous()
    wps_s, bps = ops.split_records(wps), bT.repeat(s * s)
    xa = x.reshape(M0, C)
    sc0 = torch.empty(ops.x3_scratch_numel(M0, C), device=D)
    u = torch.empty(Fr, h * s, w * s, C, device=D)
    wsl = wrn.permute(0, 2, 3, 1).reshape(Co, 3, 3, C // 32, 32).permute(0, 3, 1, 2, 4).reshape(Co, 9 * C).contiguous()
    wsl_s = ops.split_records(wsl)
    sc1 = torch.empty(ops.x3_scratch_numel(M1, C), device=D)
    o_unf, r_unf = torch.empty(M1, Co, device=D), ops.records_buffer(M1, Co)
    conv = dict(N=Fr, H=h * s, W=w * s, C=C, KH=3, KW=3, stride=1, pad=1, dil=1, OH=h * s, OW=w * s, slice_major=True)

    def unfolded(xa=xa, wps=wps, wps_s=wps_s, bps=bps, sc0=sc0, u=u, wsl=wsl, wsl_s=wsl_s, sc1=sc1, o=o_unf, r=r_unf, conv=conv,
                 C=C, s=s, M1=M1):
        ops.gemm(xa, wps, prec=PREC_BF16X3, bias=bps, pixel_shuffle=(s, C, Fr, h, w), out=u, w_split=wps_s, x3_scratch=sc0)
        ops.gemm(u.view(M1, C), wsl, prec=PREC_BF16X3, conv=conv, act=ACT_RELU, out=o, out_records=r, w_split=wsl_s, x3_scratch=sc1)

    # folded
    rec, beta = ops.dpt_fold_pack(wT, bT, wrn)
    ar = ops.records_buffer(M0, C)
    ar[:M0 * C * 2] = ops.split_records(xa.contiguous()).reshape(-1)
    ar[M0 * C * 2:] = 0
    o_f, r_f = torch.empty(Fr, h * s, w * s, Co, device=D), ops.records_buffer(M1, Co)

    def folded(ar=ar, rec=rec, beta=beta, o=o_f, r=r_f, C=C, s=s):
        ops.convT_conv3x3_folded((Fr, h, w, C), rec, beta, s, Co, act=ACT_RELU, out=o, out_records=r, a_records=ar)

    unfolded(); folded()
    torch.cuda.synchronize()
    d = (o_f.view(M1, Co) - o_unf).abs().max().item() / o_unf.abs().max().item()
    print(f"level {lvl}: folded vs unfolded max abs difference / max abs value {d:.2e}", flush=True)
    fns[(lvl, "unfolded")], fns[(lvl, "folded")] = unfolded, folded
    taps = (s + 2) ** 2
    flops[(lvl, "unfolded")] = 2.0 * M0 * C * s * s * C + 2.0 * M1 * 9 * C * Co
    flops[(lvl, "folded")] = 2.0 * M0 * taps * C * Co
res = {k: [] for k in fns}
for rep in range(int(os.environ.get("AB_REPS", 5))):
    for k in fns:
        res[k].append(timeit(fns[k], iters=10, warm=2))
for lvl in (0, 1):
    med = {}
    for v in ("unfolded", "folded"):
        ts = sorted(res[(lvl, v)])
        med[v] = ts[len(ts) // 2]
        print(f"level {lvl} {v:8s}: median {med[v] * 1e6:8.1f} us  {3 * flops[(lvl, v)] / med[v] / 1e12:6.0f} TF/s of MFMA work  (min {ts[0] * 1e6:.1f})",
              flush=True)
    print(f"level {lvl} unfolded -> folded: {100 * (med['folded'] / med['unfolded'] - 1):+.1f} %", flush=True)
