"""Side measurement: per-step time of DDIM inversion against the DDIM sampling loop, at the headline shape.

  python tools/invert_bench.py [--model Latte-XL/2] [--batch 8] [--steps 20] [--reps 5] [--out profiles/invert.json]

Latte-XL/2, 16 frames of 32x32 latents, B = 8, f16 operands, random weights, create_diffusion("250").  Three loops over the SAME
`steps` respaced indices (250 - steps ... 249), interleaved in one process, device events around each whole loop, medians of `reps`
repetitions after one warm-up loop of each:
  invert_fused     latte_invert_loop, ascending, unguided
  ddim             latte_sample_loop, DDIM eta 0, unguided, descending -- the existing sampling loop, the yardstick
  invert_stepwise  the step-by-step Python path of ddim_reverse_sample_loop (model.forward, latte_sampler_step_ex per step)
An inversion step is a DDIM step: the same forward on the same chain conditioning and the same update kernel with two other
coefficients, so the ratio is expected at 1 within the spread the same measurement showed for latte_bpd_loop (0.999 and 1.0012 on
two boxes, profiles/bpd.json).  The box is named in the file."""
import argparse
import json
import os
import socket
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import latte_amd  # noqa: E402
from latte_amd._lib import check, load_library, ptr, stream_ptr  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="Latte-XL/2")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--input-size", type=int, default=32)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "invert.json"))
    a = ap.parse_args()
    torch.set_grad_enabled(False)
    if not torch.cuda.is_available():
        raise SystemExit("tools/invert_bench.py needs an MI355X")
    B = a.batch
    m = latte_amd.Latte_models[a.model](input_size=a.input_size, num_frames=a.frames, num_classes=101, extras=2, learn_sigma=True,
                                        compute_dtype="f16", max_batch=B)
    g = torch.Generator("cpu").manual_seed(1)
    for _, p in m.named_parameters():        # the zero-initialised gates and final layer re-drawn: every block reaches the output
        if p.requires_grad and float(p.detach().abs().max()) == 0.0:
            p.copy_(torch.randn(p.shape, generator=g) * 0.02)
    m = m.cuda().eval()
    d = latte_amd.create_diffusion("250")
    n = d.num_timesteps
    hi, lo = n - 1, n - a.steps
    x0 = (torch.randn(B, a.frames, 4, a.input_size, a.input_size, generator=g) * 0.6).clamp(-1, 1).cuda()
    y = torch.randint(0, 101, (B,), generator=g).cuda()
    lib, eng = load_library(), m.engine(B)
    x, xi = torch.empty_like(x0), torch.empty_like(x0)

    def invert_fused():
        xi.copy_(x0)
        check(lib.latte_invert_loop(eng, d._h, 0, 0, 1.0, ptr(xi), ptr(y), B, lo, hi, None, None, stream_ptr()))

    def ddim():
        x.copy_(x0)
        check(lib.latte_sample_loop(eng, d._h, 1, 0.0, 0, 1.0, ptr(x), ptr(y), B, hi, lo, None, None, None, stream_ptr()))

    stepped = {}

    def invert_stepwise():      # a plain callable: the generic path of ddim_reverse_sample_loop
        stepped["x"] = d.ddim_reverse_sample_loop(lambda xx, tt, **k: m.forward(xx, tt, **k), x0, clip_denoised=False, model_kwargs=dict(y=y),
                                                  start_index=lo, end_index=hi)

    loops = {"invert_fused": invert_fused, "ddim": ddim, "invert_stepwise": invert_stepwise}

    def timed(fn):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / a.steps

    print("model ready, warm-up", flush=True)
    for fn in loops.values():
        timed(fn)
    ms = {k: [] for k in loops}
    for r in range(a.reps):
        for k, fn in loops.items():          # interleaved
            ms[k].append(timed(fn))
        print("  rep %d: " % r + ", ".join("%s %.3f" % (k, v[-1]) for k, v in ms.items()) + " ms per step", flush=True)
    med = {k: statistics.median(v) for k, v in ms.items()}
    same = float((stepped["x"] - xi).norm() / xi.norm())
    result = {"what": "ms per step of latte_invert_loop, of the unguided DDIM latte_sample_loop and of ddim_reverse_sample_loop's step-by-step path "
                      "over the same respaced indices of create_diffusion('250'); device events around whole loops, medians of `reps` "
                      "interleaved repetitions after one warm-up loop of each",
              "model": a.model, "latent": [a.frames, 4, a.input_size, a.input_size], "batch": B, "operands": "f16", "steps_per_loop": a.steps,
              "reps": a.reps, "device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName, "box": socket.gethostname(),
              "ms_per_step": ms, "median_ms_per_step": med,
              "invert_step_over_ddim_step": med["invert_fused"] / med["ddim"],
              "stepwise_over_fused": med["invert_stepwise"] / med["invert_fused"],
              "spread_of_the_yardstick": (max(ms["ddim"]) - min(ms["ddim"])) / med["ddim"],
              "stepwise_vs_fused_rel_l2": same,
              "finite": bool(torch.isfinite(xi).all() and torch.isfinite(x).all())}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({k: result[k] for k in ("median_ms_per_step", "invert_step_over_ddim_step", "stepwise_over_fused", "stepwise_vs_fused_rel_l2", "finite", "box")}))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
