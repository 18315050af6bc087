#!/usr/bin/env python3
"""Is the device assembly of every csrc/*.hip the parent's?  The proof of a refactor that must not move the kernels.

    python tools/asm_diff.py <parent-rev> [file.hip ...] [--jobs N] [--keep DIR]

Compiles every `.hip` under `csrc` (or the named ones) twice -- at <parent-rev>, whose `csrc` and `include` are
extracted with `git archive` into a temporary directory, and in the working tree -- with build.py's own CXXFLAGS and
EXTRA_FLAGS plus `--cuda-device-only -S`, and compares the two texts, ignoring only lines that contain `__hip_cuid_`
(a hash of the source text) and the `.file` directive.  The compiler's diagnostics are compared as well, with the two
directory names taken out.  One line per file: assembly line count, then `identical` or the number of differing
lines; a file that only the working tree has is compiled and listed as `new file` with its line count (a host-only
file is the 23-line stub).  Exits non-zero if any file differs or only the parent has it.  Needs hipcc and git, no
GPU; nothing inside the assembly is inspected.
`--keep DIR` leaves parent/<name>.s and tree/<name>.s there (and reuses a parent/<name>.s it finds: the parent's
output does not change while one edits).
"""
from __future__ import annotations

import argparse
import difflib
import io
import subprocess
import sys
import tarfile
import tempfile
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from skiing_analysis_pytorch_amd.build import CSRC, CXXFLAGS, EXTRA_FLAGS, HIPCC  # noqa: E402

CSRC_REL = CSRC.relative_to(ROOT).as_posix()


def extract_parent(rev: str, dst: Path) -> Path:
    tar = subprocess.run(["git", "-C", str(ROOT), "archive", rev, CSRC_REL, "include"], check=True,
                         capture_output=True).stdout
    tarfile.open(fileobj=io.BytesIO(tar)).extractall(dst)
    return dst / CSRC_REL


def compile_asm(src: Path, out: Path) -> str:
    """Writes the device assembly of `src` to `out`; returns the diagnostics without the source directory's name."""
    cmd = [HIPCC, *CXXFLAGS, *EXTRA_FLAGS.get(src.name, []), "--cuda-device-only", "-S", str(src), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit(f"hipcc failed for {src}:\n{r.stdout}\n{r.stderr}")
    return (r.stdout + r.stderr).replace(str(src.parent) + "/", "")


def kept_lines(path: Path) -> list[str]:
    return [l for l in path.read_text().splitlines() if "__hip_cuid_" not in l and not l.lstrip().startswith(".file")]


def differing(a: list[str], b: list[str]) -> int:
    if a == b:
        return 0
    return sum(1 for l in difflib.ndiff(a, b) if l[:2] in ("- ", "+ ")) if max(len(a), len(b)) < 4000 else \
        sum(1 for l in difflib.unified_diff(a, b, n=0, lineterm="") if l[:1] in "+-" and l[:3] not in ("+++", "---"))


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("parent", help="revision to compare the working tree with")
    ap.add_argument("files", nargs="*", help="names of csrc/*.hip files (default: all, and those only the parent has)")
    ap.add_argument("--jobs", type=int, default=4)
    ap.add_argument("--keep", type=Path, help="directory for the .s files (default: a temporary one)")
    args = ap.parse_args()

    with tempfile.TemporaryDirectory() as tmp:
        work = args.keep.resolve() if args.keep else Path(tmp)
        pdir, tdir = work / "parent", work / "tree"
        pdir.mkdir(parents=True, exist_ok=True)
        tdir.mkdir(parents=True, exist_ok=True)
        pcsrc = extract_parent(args.parent, Path(tmp) / "src")
        names = args.files or sorted({p.name for p in CSRC.glob("*.hip")} | {p.name for p in pcsrc.glob("*.hip")})

        def one(name: str):
            res = []
            if not (pcsrc / name).exists():   # new in the tree: its line count shows whether it holds device code at all
                (tdir / (name + ".diag")).write_text(compile_asm(CSRC / name, tdir / (name + ".s")))
                return name, len(kept_lines(tdir / (name + ".s"))), None, True
            for csrc, out in ((pcsrc, pdir), (CSRC, tdir)):
                s, diag = out / (name + ".s"), out / (name + ".diag")
                if not (csrc / name).exists():
                    return name, None, None, None
                if not (out is pdir and args.keep and s.exists() and diag.exists()):
                    diag.write_text(compile_asm(csrc / name, s))
                res.append((kept_lines(s), diag.read_text()))
            (pa, pd), (ta, td) = res
            return name, len(ta), differing(pa, ta), pd == td

        bad = 0
        with ThreadPoolExecutor(max_workers=args.jobs) as ex:
            for name, n, d, same_diag in ex.map(one, names):
                if n is None:
                    print(f"{name:24s} only on one side")
                    bad += 1
                    continue
                if d is None:
                    print(f"{name:24s} {n:7d} lines  new file", flush=True)
                    continue
                verdict = "identical" if d == 0 else f"{d} lines differ"
                if not same_diag:
                    verdict += ", diagnostics differ"
                print(f"{name:24s} {n:7d} lines  {verdict}", flush=True)
                bad += d != 0 or not same_diag
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
