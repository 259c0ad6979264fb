#!/usr/bin/env python
"""Milliseconds per joint image-video training step (LatteTrainer(use_image_num=N)) beside two plain steps, in one process:

  joint      Latte-B/2, 32 x 32 latents, F = 16 video frames + N = 8 images per sample, batch 4, f16 operands
  video      the plain step on the same model: batch 4, F = 16
  frames24   the plain step of a model with num_frames = 24, batch 4: as many frames through the spatial blocks and the final layer
             as the joint step, and its temporal blocks run over all 24 -- strictly more work than the joint step

Each step is forward + backward + clip + AdamW + EMA on fixed inputs (train_step with t / noise given).  Per variant: `--warmup`
steps, then `--repeats` timed groups of `--steps` steps between two events; the median group and the spread are reported.
Unconditional models (configs/ffs_img_train.yaml).  Writes one JSON object to --out.

    python tools/train_joint_bench.py --out profiles/train_joint.json"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import latte_amd  # noqa: E402


def measure(name, frames, images, batch, latent, steps, warmup, repeats, dtype):
    torch.manual_seed(0)
    model = latte_amd.Latte_models[name](input_size=latent, num_frames=frames, learn_sigma=True, extras=1).to("cuda")
    tr = latte_amd.LatteTrainer(model, latte_amd.create_diffusion(""), max_batch=batch, compute_dtype=dtype, use_image_num=images)
    g = torch.Generator("cuda").manual_seed(1)
    x = torch.randn(batch, frames + images, 4, latent, latent, device="cuda", generator=g)
    noise = torch.randn(x.shape, device="cuda", generator=g)
    t = torch.randint(0, 1000, (batch,), device="cuda", generator=g)
    for _ in range(warmup):
        tr.train_step(x, t=t, noise=noise)
    torch.cuda.synchronize()
    groups = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            out = tr.train_step(x, t=t, noise=noise)
        b.record()
        torch.cuda.synchronize()
        groups.append(a.elapsed_time(b) / steps)
    sc = tr.scaler_state()
    res = {"frames": frames, "images": images, "batch": batch, "ms_per_step": statistics.median(groups), "ms_min": min(groups),
           "ms_max": max(groups), "groups": groups, "loss": float(out["loss"].mean()), "skipped_updates": sc["skipped_updates"]}
    del tr, model
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="Latte-B/2")
    ap.add_argument("--latent", type=int, default=32)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--dtype", default="f16")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "tools/train_joint_bench.py needs an MI355X"
    kw = dict(batch=a.batch, latent=a.latent, steps=a.steps, warmup=a.warmup, repeats=a.repeats, dtype=a.dtype)
    res = {"model": a.model, "latent": a.latent, "dtype": a.dtype, "steps_per_group": a.steps, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0)}
    # interleaved order twice would cost three more trainers; the variants run one after the other, the first one again at the end
    res["video"] = measure(a.model, a.frames, 0, **kw)
    res["joint"] = measure(a.model, a.frames, a.images, **kw)
    res["frames24"] = measure(a.model, a.frames + a.images, 0, **kw)
    res["video_again"] = measure(a.model, a.frames, 0, **kw)
    j, v, w = res["joint"]["ms_per_step"], res["video"]["ms_per_step"], res["frames24"]["ms_per_step"]
    res["joint_over_video"] = j / v
    res["joint_over_frames24"] = j / w
    res["drift_video"] = res["video_again"]["ms_per_step"] / v
    res["expected"] = "joint <= 1.03 * frames24 (the step of F + N frames does strictly more work: its temporal blocks see all of them)"
    res["met"] = bool(j <= 1.03 * w)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
