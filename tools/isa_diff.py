#!/usr/bin/env python3
"""Compare the gfx950 device assembly of every .hip in build.py's SOURCES between a git revision and the working tree.

    python tools/isa_diff.py [<rev>] [file.hip ...]        (default rev: HEAD; default files: all)

Each revision compiles with its own headers, with build.py's .hip flags plus --cuda-device-only -S, once with the product flags and once
with -DLATTE_GEMM_ABLATE (the measurement build).  Lines that mention the per-compile __hip_cuid_ symbol are dropped.  A refactor of the
kernels that claims "device code unchanged" shows a table of "same" here; exit status 1 otherwise.  Needs hipcc, no GPU.
"""
import io
import os
import subprocess
import sys
import tarfile
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from latte_amd import build as B  # noqa: E402

BASE_FLAGS = [f for f in B.FLAGS[".hip"] if f != "-DLATTE_GEMM_ABLATE"]
VARIANTS = {"product": [], "ablate": ["-DLATTE_GEMM_ABLATE"]}


def asm(tree, name, extra):
    # cwd = the source's directory and a relative path: nothing in the output names the tree
    cmd = [B.HIPCC] + BASE_FLAGS + extra + ["--cuda-device-only", "-S", name, "-o", "-"]
    r = subprocess.run(cmd, cwd=os.path.join(tree, "latte_amd", "csrc"), capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("hipcc failed for %s in %s:\n%s" % (name, tree, r.stderr[-4000:]))
    return [line for line in r.stdout.splitlines() if "__hip_cuid_" not in line]


def main(argv):
    files = [a for a in argv if a.endswith(".hip")]
    revs = [a for a in argv if not a.endswith(".hip")]
    rev = revs[0] if revs else "HEAD"
    files = files or [s for s in B.SOURCES if s.endswith(".hip")]
    with tempfile.TemporaryDirectory() as old:
        tar = subprocess.run(["git", "archive", rev, "latte_amd/csrc", "include"], cwd=ROOT, capture_output=True, check=True).stdout
        tarfile.open(fileobj=io.BytesIO(tar)).extractall(old)
        jobs = [(tree, f, v) for f in files for v in VARIANTS for tree in (old, ROOT)]
        with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
            out = dict(zip(jobs, ex.map(lambda j: asm(j[0], j[1], VARIANTS[j[2]]), jobs)))
    bad = 0
    print("%-16s %-8s %9s  %s" % ("file", "build", "asm lines", "vs " + rev))
    for f in files:
        for v in VARIANTS:
            a, b = out[(old, f, v)], out[(ROOT, f, v)]
            bad += a != b
            print("%-16s %-8s %9d  %s" % (f, v, len(b), "same" if a == b else "DIFFERENT"))
    print("%d of %d comparisons match" % (len(files) * len(VARIANTS) - bad, len(files) * len(VARIANTS)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
