#!/usr/bin/env python
"""Writes tests/golden/bpd.npz: likelihood evaluation (gaussian_diffusion.py:813-866 calc_bpd_loop, :686-717 _vb_terms_bpd,
:797-811 _prior_bpd) run by the REFERENCE objects.

Needs the reference checkout (LATTE_REFERENCE_ROOT); tests/bpd_reference.py:reference_arrays loads models/latte.py and diffusion/
by path, unmodified, through oracle.reference_loader (the tools themselves do not import the oracle).  Fixture M is the reference's
own ``calc_bpd_loop`` on the reference's Latte with weights from ``oracle.latte_oracle.init_state_dict``; fixtures K are its
``_vb_terms_bpd`` / ``_predict_eps_from_xstart`` / ``_prior_bpd`` on the synthetic model's outputs.

The file holds numbers only: the per-sample terms the reference computed, and for every regenerated random input (seeded CPU
generators, tests/bpd_reference.py) its sum and first eight values -- so a drift of the CPU generator shows as "inputs differ",
not as a parity miss.  No tensor is stored.

    python tools/make_bpd_golden.py [--check]      # --check: compare with the committed file instead of writing"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
OUT = os.path.join(ROOT, "tests", "golden", "bpd.npz")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    import bpd_reference as br
    arrays = br.reference_arrays()
    if args.check:
        z = np.load(OUT)
        assert set(z.files) == set(arrays), sorted(set(z.files) ^ set(arrays))
        bad = [k for k in arrays if k.startswith("in::") and not np.array_equal(z[k], arrays[k])]
        if bad:
            print("inputs differ (the seeded CPU generators no longer give the fixture's inputs):", bad)
            return 1
        worst = max(float((np.abs(z[k] - arrays[k]) / np.maximum(np.abs(arrays[k]), 1e-30)).max()) for k in arrays)
        print("worst relative difference to the committed fixture:", worst)
        return 0 if worst < 1e-5 else 1
    np.savez_compressed(OUT, **arrays)
    print(OUT, os.path.getsize(OUT), "bytes,", len(arrays), "arrays")
    return 0


if __name__ == "__main__":
    sys.exit(main())
