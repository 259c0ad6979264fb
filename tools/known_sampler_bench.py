"""Side measurement: per-step time of known-region sampling against the unchanged DDIM sampling loop, at the headline shape.

  python tools/known_sampler_bench.py [--model Latte-XL/2] [--batch 8] [--steps 20] [--reps 5] [--out profiles/known_sampler.json]
                                      [--bench-line FILE --parent-bench-line FILE]

Latte-XL/2, 16 frames of 32x32 latents, B = 8, f16 operands, random weights, create_diffusion("250"), DDIM eta 0, the first frame
known.  Three loops over the SAME `steps` respaced indices (249 ... 250 - steps), interleaved in one process, device events around
each whole loop, medians of `reps` repetitions after one warm-up loop of each:
  known_fused     SpacedDiffusion.known_sample_loop on model.forward: ONE latte_sample_loop_known call (explicit slabs)
  ddim            SpacedDiffusion.ddim_sample_loop on model.forward: ONE latte_sample_loop_ex call -- the unchanged loop, the yardstick
  known_stepwise  the step-by-step Python path of known_sample_loop (a plain callable: model.forward, latte_sampler_step_ex and
                  latte_known_blend per step)
A known-region step is a DDIM step plus one blend launch that reads the known clip, a noise slab and the mask and rewrites a
sixteenth of x: about 7 MB beside a 30 ms forward, so the ratio is expected at 1 within the spread of the interleaved repeats, where
the other fused chains sit (README: 0.9995 - 1.004).  --bench-line / --parent-bench-line: files holding the JSON result line of a
default ``bench.py --gpus 1`` run on this commit and on its parent; both are recorded in the output.  The box is named in the file."""
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


def last_json_line(path):
    with open(path) as f:
        lines = [ln for ln in f.read().splitlines() if ln.strip().startswith("{")]
    return json.loads(lines[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="Latte-XL/2")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--input-size", type=int, default=32)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--bench-line", default="")
    ap.add_argument("--parent-bench-line", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "known_sampler.json"))
    a = ap.parse_args()
    torch.set_grad_enabled(False)
    if not torch.cuda.is_available():
        raise SystemExit("tools/known_sampler_bench.py needs an MI355X")
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
    shape = (B, a.frames, 4, a.input_size, a.input_size)
    known = (torch.randn(shape, generator=g) * 0.6).clamp(-1, 1).cuda()
    z = torch.randn(shape, generator=g).cuda()
    y = torch.randint(0, 101, (B,), generator=g).cuda()
    mask = latte_amd.known_mask(shape, frames=[0]).cuda()
    slabs = torch.randn((d.known_chain_slabs("ddim", start_index=hi, end_index=lo),) + shape, generator=g).cuda()
    kw = dict(noise=z, clip_denoised=False, model_kwargs=dict(y=y), start_index=hi, end_index=lo)
    out = {}

    def known_fused():
        out["fused"] = d.known_sample_loop(m.forward, shape, known, mask, chain_noise=slabs, **kw)

    def ddim():
        out["ddim"] = d.ddim_sample_loop(m.forward, shape, **kw)

    def known_stepwise():
        out["stepwise"] = d.known_sample_loop(lambda xx, tt, **k: m.forward(xx, tt, **k), shape, known, mask, chain_noise=slabs, **kw)

    loops = {"known_fused": known_fused, "ddim": ddim, "known_stepwise": known_stepwise}

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
    same = float((out["stepwise"] - out["fused"]).norm() / out["fused"].norm())
    result = {"what": "ms per step of SpacedDiffusion.known_sample_loop (DDIM, first frame known) as one latte_sample_loop_known call, of the "
                      "unchanged ddim_sample_loop and of known_sample_loop's step-by-step path over the same respaced indices of "
                      "create_diffusion('250'); device events around whole loops, medians of `reps` interleaved repetitions after one "
                      "warm-up loop of each",
              "model": a.model, "latent": [a.frames, 4, a.input_size, a.input_size], "batch": B, "operands": "f16", "steps_per_loop": a.steps,
              "reps": a.reps, "device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName, "box": socket.gethostname(),
              "ms_per_step": ms, "median_ms_per_step": med,
              "known_step_over_ddim_step": med["known_fused"] / med["ddim"],
              "ratio_per_repetition": [k_ / d_ for k_, d_ in zip(ms["known_fused"], ms["ddim"])],
              "stepwise_over_fused": med["known_stepwise"] / med["known_fused"],
              "spread_of_the_yardstick": (max(ms["ddim"]) - min(ms["ddim"])) / med["ddim"],
              "spread_of_the_known_chain": (max(ms["known_fused"]) - min(ms["known_fused"])) / med["known_fused"],
              "stepwise_vs_fused_rel_l2": same,
              "known_part_exact": bool(torch.equal(out["fused"][:, 0], known[:, 0])) if lo == 0 else None,
              "finite": bool(torch.isfinite(out["fused"]).all() and torch.isfinite(out["ddim"]).all())}
    if a.bench_line:
        result["bench_this_commit"] = last_json_line(a.bench_line)
    if a.parent_bench_line:
        result["bench_parent_commit"] = last_json_line(a.parent_bench_line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({k: result[k] for k in ("median_ms_per_step", "known_step_over_ddim_step", "stepwise_over_fused", "spread_of_the_yardstick",
                                             "stepwise_vs_fused_rel_l2", "finite", "box")}))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
