"""The tail of a DPT head at the bench batch (32 frames, 296 x 296 -> 518 x 518, 128 -> 32 channels, UV tables): the
align-corners upsample into pixel records followed by the direct 3 x 3 conv (SKIMI_DPT_TAIL_FUSED=0: two launches, 4.4 GB of
records written and read back) against the conv that interpolates its own windows (=1: one launch, no records).
Interleaved A/B inside one process (SKIMI_ENV_DYNAMIC=1), median over the repeats, the outputs compared bit for bit."""
import ctypes as C
import os
import statistics
import sys
from pathlib import Path

os.environ["SKIMI_ENV_DYNAMIC"] = "1"
import torch  # noqa: E402

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from skiing_analysis_pytorch_amd import _lib  # noqa: E402
from skiing_analysis_pytorch_amd._lib import check, lib, ptr  # noqa: E402
from tools.microbench import timeit  # noqa: E402

F_, h, w, H, W, Cc = 32, 296, 296, 518, 518, 128
REPEATS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
src = torch.randn((F_, h, w, Cc), device="cuda")
tabx, taby = 0.1 * torch.randn((W, Cc // 2), device="cuda"), 0.1 * torch.randn((H, Cc // 2), device="cuda")
wt = torch.randn((32, Cc, 3, 3), device="cuda") / (9 * Cc) ** 0.5
packed = torch.empty(2 * 32 * Cc * 9, dtype=torch.bfloat16, device="cuda")
st = _lib.current_stream()
check(lib().skimi_conv3x3_n32_pack(ptr(wt), ptr(packed), Cc, st), "pack")
bias = torch.randn(32, device="cuda")
rec = torch.empty((F_, H, W, 2 * Cc), dtype=torch.bfloat16, device="cuda")
outs = {m: torch.empty((F_, H, W, 32), device="cuda") for m in (0, 1)}


def run(mode):
    os.environ["SKIMI_DPT_TAIL_FUSED"] = str(mode)
    fused = C.c_int32(-1)
    check(lib().skimi_conv3x3_n32_upsampled(ptr(src), h, w, ptr(tabx), ptr(taby), ptr(packed), ptr(bias), ptr(outs[mode]), F_, H, W,
                                            Cc, 1, ptr(rec), C.byref(fused), st), "tail")
    assert fused.value == mode


times = {0: [], 1: []}
for _ in range(REPEATS):
    for mode in (0, 1):
        times[mode].append(timeit(lambda: run(mode), iters=10))
torch.cuda.synchronize()
for mode in (0, 1):
    t = statistics.median(times[mode])
    print(f"DPT tail x {F_}, SKIMI_DPT_TAIL_FUSED={mode}: median {t*1e6:.0f} us (min {min(times[mode])*1e6:.0f}, max "
          f"{max(times[mode])*1e6:.0f})")
print(f"ratio 0 / 1: {statistics.median(times[0]) / statistics.median(times[1]):.3f}; "
      f"outputs bit-identical: {torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))}")
