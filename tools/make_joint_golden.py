#!/usr/bin/env python
"""Writes tests/golden/train_joint.npz: one joint image-video micro-batch (train_with_img.py:214-241) run by the REFERENCE objects.

Needs the reference checkout (LATTE_REFERENCE_ROOT); tests/joint_reference.py:reference_step loads models/latte_img.py by path,
unmodified, on oracle.reference_loader's timm stand-in, and diffusion/ as it is (the tools themselves do not import the oracle).  ``LatteIMG(...).train()`` is built with class_dropout_prob 0.1 (the label table has its null
row), ``y_embedder.dropout_prob`` is then set to 0 on the instance and the dropped labels are passed as ``num_classes`` --
``token_drop`` does exactly that replacement.  ``create_diffusion("").training_losses`` and ``loss.mean().backward()`` follow.

The weights come from ``oracle.latte_oracle.init_state_dict`` (tests/joint_reference.py:joint_inputs), so the file holds only what the
reference computed, as numeric arrays: the terms, the model output, and per gradient tensor its L2 norm and the elements at
``joint_reference.sample_index`` (every element of a tensor up to GOLD_SAMPLE elements).

    python tools/make_joint_golden.py [--check]      # --check: compare with the committed file instead of writing"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
OUT = os.path.join(ROOT, "tests", "golden", "train_joint.npz")


def fixture_arrays():
    import joint_reference as jr
    cfg, sd, x0, noise, t, y, y_image, drop, image_drop = jr.joint_inputs()
    terms, out, grads = jr.reference_step(jr.J_MODEL, sd, x0, noise, t, y, y_image, drop, image_drop, jr.J_IMAGES)
    arrays = {f"terms::{k}": v.numpy() for k, v in terms.items()}
    arrays["model_out"] = out.numpy()
    for k, g in grads.items():
        arrays[f"gnorm::{k}"] = np.float64(g.double().norm().item())
        arrays[f"gsample::{k}"] = g.reshape(-1)[jr.sample_index(g.numel())].numpy()
    return arrays


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    arrays = fixture_arrays()
    if args.check:
        z = np.load(OUT)
        assert set(z.files) == set(arrays), sorted(set(z.files) ^ set(arrays))
        worst = max(float(np.abs(z[k] - arrays[k]).max() / (np.abs(arrays[k]).max() + 1e-30)) for k in arrays)
        print("worst relative difference to the committed fixture:", worst)
        return 0 if worst < 1e-5 else 1
    np.savez(OUT, **arrays)
    print(OUT, os.path.getsize(OUT), "bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
