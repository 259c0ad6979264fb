"""Side measurement: per-step time of likelihood evaluation against the DDIM sampling loop, at the headline shape.

  python tools/bpd_bench.py [--model Latte-XL/2] [--batch 8] [--steps 20] [--reps 5] [--out profiles/bpd.json]

Latte-XL/2, 16 frames of 32x32 latents, B = 8, f16 operands, random weights, create_diffusion("250").  Three loops over the SAME
`steps` respaced indices (249 ... 250 - steps), interleaved in one process, device events around each whole loop, medians of `reps`
repetitions after one warm-up loop of each:
  bpd_fused     latte_bpd_loop (noise from the engine's Philox stream)
  ddim          latte_sample_loop, DDIM eta 0, unguided -- the existing sampling loop, the yardstick
  bpd_stepwise  the step-by-step Python path of calc_bpd_loop's (q_sample, model.forward, latte_bpd_terms per step)
A bpd step is a DDIM step whose sampler update is replaced by a noise fill, q_sample and the terms kernel with its finalize pass:
about 36 bytes per latent element (19 MB per step at this shape) beside a ~30 ms forward, so the ratio is expected inside the
+- 3 % spread between boxes (README).  The box is named in the file."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bpd.json"))
    a = ap.parse_args()
    torch.set_grad_enabled(False)
    if not torch.cuda.is_available():
        raise SystemExit("tools/bpd_bench.py needs an MI355X")
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
    tabs = tuple(torch.empty(B, a.steps, device="cuda") for _ in range(3))
    x = torch.empty_like(x0)

    def bpd_fused():
        check(lib.latte_bpd_loop(eng, d._h, 1, ptr(x0), ptr(y), B, hi, lo, None, ptr(tabs[0]), ptr(tabs[1]), ptr(tabs[2]), stream_ptr()))

    def ddim():
        x.copy_(x0)
        check(lib.latte_sample_loop(eng, d._h, 1, 0.0, 0, 1.0, ptr(x), ptr(y), B, hi, lo, None, None, None, stream_ptr()))

    def bpd_stepwise():
        for k, i in enumerate(range(hi, lo - 1, -1)):
            nz = torch.randn_like(x0)
            x_t = d.q_sample(x0, torch.full((B,), i, device="cuda", dtype=torch.int64), nz)
            out = m.forward(x_t, torch.full((B,), d.timestep_map[i], device="cuda", dtype=torch.int64), y=y)
            d._bpd_terms(x0, x_t, nz, out, i, True, tabs, k)

    loops = {"bpd_fused": bpd_fused, "ddim": ddim, "bpd_stepwise": bpd_stepwise}

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
    per_step_bytes = 36 * x0.numel()
    result = {"what": "ms per step of latte_bpd_loop, of the unguided DDIM latte_sample_loop and of calc_bpd_loop's step-by-step path "
                      "over the same respaced indices of create_diffusion('250'); device events around whole loops, medians of `reps` "
                      "interleaved repetitions after one warm-up loop of each",
              "model": a.model, "latent": [a.frames, 4, a.input_size, a.input_size], "batch": B, "operands": "f16", "steps_per_loop": a.steps,
              "reps": a.reps, "device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName, "box": socket.gethostname(),
              "ms_per_step": ms, "median_ms_per_step": med,
              "bpd_step_over_ddim_step": med["bpd_fused"] / med["ddim"],
              "stepwise_over_fused": med["bpd_stepwise"] / med["bpd_fused"],
              "spread_of_the_yardstick": (max(ms["ddim"]) - min(ms["ddim"])) / med["ddim"],
              "non_forward_bytes_per_step_expected": per_step_bytes,
              "finite": bool(all(torch.isfinite(t).all() for t in tabs))}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({k: result[k] for k in ("median_ms_per_step", "bpd_step_over_ddim_step", "stepwise_over_fused", "box")}))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
