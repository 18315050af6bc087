# max abs / max relative difference per array between two bench.py --dump-outputs directories
import sys
from pathlib import Path
import numpy as np
a, b = Path(sys.argv[1]), Path(sys.argv[2])
for f in sorted(a.glob("*.npy")):
    x, y = np.load(f).astype(np.float64), np.load(b / f.name).astype(np.float64)
    d = np.abs(x - y)
    rel = d.max() / max(np.abs(y).max(), 1e-30)
    print(f"{f.stem:40s} {str(x.shape):20s} max abs diff {d.max():.3e}  rel to max|x| {rel:.3e}  differing {int((d > 0).sum())} / {d.size}")
