#!/usr/bin/env python
"""Writes tests/golden/invert.npz: DDIM inversion (gaussian_diffusion.py:566-602 ddim_reverse_sample) run by the REFERENCE objects.

Needs the reference checkout (LATTE_REFERENCE_ROOT); tests/invert_reference.py:reference_arrays loads models/latte.py and diffusion/
by path, unmodified, through oracle.reference_loader (the tools themselves do not import the oracle).  Fixture M is the reference's
own ``ddim_reverse_sample`` stepped ``for i in range(50)`` on the reference's Latte with weights from
``oracle.latte_oracle.init_state_dict`` (``forward``, clip_denoised on and off, and ``forward_with_cfg`` at scale 4.0 on the doubled
batch); fixtures K are single reverse steps on the synthetic model's outputs.

Everything is computed on ONE CPU thread (tests/invert_reference.py:one_thread) and on MKL's vendor-neutral code path: the tool
runs itself in a child with MKL_CBWR=COMPATIBLE, the arithmetic tests/_util.pinned reproduces on every x86 host.  MKL's default
path depends on the CPU: on the host that wrote the fixture the oracle's chain and the reference's agree bit for bit on it, on
another host the same restatement differed from that fixture in the seventh digit.

The file holds numbers only: a few checkpoints of each chain, per kernel-level case a few evenly spaced elements and the sums of the
result, and for every regenerated random input (seeded CPU generators, tests/bpd_reference.py) its sum and first eight values.

    python tools/make_invert_golden.py [--check]      # --check: compare with the committed file instead of writing"""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
OUT = os.path.join(ROOT, "tests", "golden", "invert.npz")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    if os.environ.get("MKL_CBWR") != "COMPATIBLE":      # MKL reads it at its first call: a fresh process
        return subprocess.run([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=dict(os.environ, MKL_CBWR="COMPATIBLE")).returncode
    import invert_reference as ir
    arrays = ir.reference_arrays()
    if args.check:
        z = np.load(OUT)
        assert set(z.files) == set(arrays), sorted(set(z.files) ^ set(arrays))
        bad = [k for k in arrays if not np.array_equal(z[k], arrays[k])]
        print("arrays that differ from the committed fixture:", bad)
        return 1 if bad else 0
    np.savez_compressed(OUT, **arrays)
    print(OUT, os.path.getsize(OUT), "bytes,", len(arrays), "arrays")
    return 0


if __name__ == "__main__":
    sys.exit(main())
