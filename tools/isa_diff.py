#!/usr/bin/env python3
"""Compare the gfx950 device assembly of every .hip in build.py's SOURCES between a git revision and the working tree, kernel by kernel.

    python tools/isa_diff.py [<rev>] [file.hip ...]        (default rev: HEAD; default files: all)

Each revision compiles with its own headers, with build.py's .hip flags plus --cuda-device-only -S.  A file's assembly is cut into one
chunk per kernel -- its code from its label to the end of its text section (s_endpgm, out-of-line blocks and padding), plus its
.amdhsa_kernel ... .end_amdhsa_kernel block -- every mangled name (_Z...) becomes a placeholder, local labels lose the index of the
function they belong to, assembler comments go, and lines that mention the per-compile __hip_cuid_ symbol are dropped; the two sorted lists of chunks are
compared.  So a refactor may rename a kernel (a dropped template argument changes the mangling) or change the order in
which instantiations are emitted; it may not change an instruction or a kernel descriptor.  A refactor of the kernels that claims
"device code unchanged" shows a table of "same" here -- "same + n new" where a file gained kernels and every kernel it had is still
there, instruction for instruction --; exit status 1 otherwise.  Needs hipcc, no GPU.
"""
import io
import os
import re
import subprocess
import sys
import tarfile
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from latte_amd import build as B  # noqa: E402

MANGLED = re.compile(r"_Z\w+")
LOCAL = re.compile(r"(\.L[A-Za-z_]+)\d+_")   # .LBB<function index>_<block>: the index is the emission order


def kernels(tree, name):
    """Sorted list of per-kernel chunks of `name` compiled in `tree`."""
    if not os.path.exists(os.path.join(tree, "latte_amd", "csrc", name)):
        return []          # a file the revision does not have yet: all of its kernels are new
    # cwd = the source's directory and a relative path: nothing in the output names the tree
    cmd = [B.HIPCC] + B.FLAGS[".hip"] + ["--cuda-device-only", "-S", name, "-o", "-"]
    r = subprocess.run(cmd, cwd=os.path.join(tree, "latte_amd", "csrc"), capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("hipcc failed for %s in %s:\n%s" % (name, tree, r.stderr[-4000:]))
    code, desc, sym = {}, {}, None   # symbol -> lines of its code / of its descriptor block; the chunk being filled
    for line in r.stdout.splitlines():
        line = line.split(";")[0].rstrip()   # assembler comments name blocks by function index too
        if not line or "__hip_cuid_" in line:
            continue
        m = re.match(r"(_Z\w+):", line)
        if m:
            sym, into = m.group(1), code
        elif line.startswith("\t.amdhsa_kernel "):
            sym, into = line.split()[1], desc
        elif line.startswith("\t.section") or line.startswith("\t.text") or line.startswith("\t.protected"):
            sym = None     # (.protected / .globl open the next symbol; .p2align padding stays with the code it follows)
        if sym is not None:
            into.setdefault(sym, []).append(LOCAL.sub(r"\1_", MANGLED.sub("_Z", line)))
            if line.startswith("\t.end_amdhsa_kernel"):
                sym = None
    return sorted("\n".join(code.get(k, []) + desc[k]) for k in desc)


def main(argv):
    files = [a for a in argv if a.endswith(".hip")]
    revs = [a for a in argv if not a.endswith(".hip")]
    rev = revs[0] if revs else "HEAD"
    files = files or [s for s in B.SOURCES if s.endswith(".hip")]
    with tempfile.TemporaryDirectory() as old:
        tar = subprocess.run(["git", "archive", rev, "latte_amd/csrc", "include"], cwd=ROOT, capture_output=True, check=True).stdout
        tarfile.open(fileobj=io.BytesIO(tar)).extractall(old)
        jobs = [(tree, f) for f in files for tree in (old, ROOT)]
        with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
            out = dict(zip(jobs, ex.map(lambda j: kernels(*j), jobs)))
    bad = 0
    print("%-16s %12s %12s  %s" % ("file", "kernels " + rev[:4], "kernels now", "vs " + rev))
    for f in files:
        a, b = out[(old, f)], out[(ROOT, f)]
        left = list(b)                   # every old kernel still there unchanged, the rest new: "same + n new"
        for k in a:
            if k in left:
                left.remove(k)
        added = len(left) if len(left) == len(b) - len(a) and len(b) > len(a) else 0
        ok = a == b or added
        bad += not ok
        print("%-16s %12d %12d  %s" % (f, len(a), len(b), "same" if a == b else ("same + %d new" % added if added else "DIFFERENT")))
    print("%d of %d files match" % (len(files) - bad, len(files)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
