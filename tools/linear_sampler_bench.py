"""Side measurement: the linear samplers (Euler, Euler-ancestral, Heun, DPM-Solver++ 2M) of the class-conditional engine at the headline
shape, against the unchanged DDIM loop.

  python tools/linear_sampler_bench.py [--model Latte-XL/2] [--batch 8] [--steps 20] [--reps 3] [--out profiles/linear_sampler.json]

Latte-XL/2, 16 frames of 32x32 latents, B = 8, f16 operands, random weights, unguided (what bench.py times).  For each method the chain
of create_diffusion(str(steps)) -- `steps` evaluations, 2 steps - 1 for Heun -- three loops interleaved in one process, device events
around each whole loop, medians of `reps` repetitions after one warm-up loop of each:
  fused     SpacedDiffusion.linear_sample_loop on model.forward: ONE latte_sample_plan_loop call
  ddim      latte_sample_loop, DDIM eta 0, the last `steps` respaced indices of create_diffusion("250") -- the yardstick
  stepwise  linear_sample_loop around a plain callable: model.forward + the scheduler's torch update per evaluation
An evaluation of the plan loop is the DDIM step's forward on the same kind of chain conditioning plus one pointwise step kernel, so
fused / ddim per evaluation is expected at 1 within the spread the same kind of run showed for the bpd and inversion loops.  Then
the wall time of a whole DPM-Solver++ chain of `steps` evaluations against a whole DDIM-250 chain, once each after the above.
No sample-quality claim: the weights are random.  The box is named in the file."""
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

METHODS = ["euler", "euler_a", "heun", "dpmsolver++"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="Latte-XL/2")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--input-size", type=int, default=32)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--ddim-steps", type=int, default=250, help="the whole DDIM chain of the wall-time comparison")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "linear_sampler.json"))
    a = ap.parse_args()
    torch.set_grad_enabled(False)
    if not torch.cuda.is_available():
        raise SystemExit("tools/linear_sampler_bench.py needs an MI355X")
    B = a.batch
    m = latte_amd.Latte_models[a.model](input_size=a.input_size, num_frames=a.frames, num_classes=101, extras=2, learn_sigma=True,
                                        compute_dtype="f16", max_batch=B)
    g = torch.Generator("cpu").manual_seed(1)
    for _, p in m.named_parameters():        # the zero-initialised gates and final layer re-drawn: every block reaches the output
        if p.requires_grad and float(p.detach().abs().max()) == 0.0:
            p.copy_(torch.randn(p.shape, generator=g) * 0.02)
    m = m.cuda().eval()
    d_lin = latte_amd.create_diffusion(str(a.steps))
    d_ddim = latte_amd.create_diffusion(str(a.ddim_steps))
    n = d_ddim.num_timesteps
    z = torch.randn(B, a.frames, 4, a.input_size, a.input_size, generator=g).cuda()
    y = torch.randint(0, 101, (B,), generator=g).cuda()
    mk = dict(y=y)
    lib, eng = load_library(), m.engine(B)
    x = torch.empty_like(z)
    evals = {k: d_lin.linear_scheduler(k).engine_plan().shape[0] for k in METHODS}
    noise = {k: torch.randn((evals[k],) + tuple(z.shape), generator=g).cuda() for k in ("euler_a",)}
    out = {}

    def fused(k):
        out["fused", k] = d_lin.linear_sample_loop(m.forward, z.shape, z, method=k, model_kwargs=mk, step_noise=noise.get(k))

    def stepwise(k):
        out["stepwise", k] = d_lin.linear_sample_loop(lambda xx, tt, **kw: m.forward(xx, tt, **kw), z.shape, z, method=k, model_kwargs=mk,
                                                      step_noise=noise.get(k))

    def ddim(steps):
        x.copy_(z)
        check(lib.latte_sample_loop(eng, d_ddim._h, 1, 0.0, 0, 1.0, ptr(x), ptr(y), B, n - 1, n - steps, None, None, None, stream_ptr()))

    def timed(fn, arg, per):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        fn(arg)
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / per

    print("model ready, warm-up", flush=True)
    for k in METHODS:
        timed(fused, k, 1)
        timed(stepwise, k, 1)
    timed(ddim, a.steps, 1)
    ms = {k: {"fused": [], "ddim": [], "stepwise": []} for k in METHODS}
    for r in range(a.reps):
        for k in METHODS:                    # interleaved
            ms[k]["fused"].append(timed(fused, k, evals[k]))
            ms[k]["ddim"].append(timed(ddim, a.steps, a.steps))
            ms[k]["stepwise"].append(timed(stepwise, k, evals[k]))
        print("  rep %d: " % r + "; ".join("%s %s" % (k, ", ".join("%s %.3f" % (c, v[-1]) for c, v in ms[k].items())) for k in METHODS)
              + " ms per evaluation", flush=True)
    med = {k: {c: statistics.median(v) for c, v in ms[k].items()} for k in METHODS}
    all_ddim = [v for k in METHODS for v in ms[k]["ddim"]]
    wall_dpm = timed(fused, "dpmsolver++", 1)
    wall_ddim = timed(ddim, n, 1)
    result = {"what": "ms per denoiser evaluation of SpacedDiffusion.linear_sample_loop as one latte_sample_plan_loop call (fused), of the unguided "
                      "DDIM latte_sample_loop over the last `steps` indices of create_diffusion('%d') (ddim) and of linear_sample_loop's "
                      "step-by-step path (stepwise); device events around whole loops, medians of `reps` interleaved repetitions after one "
                      "warm-up loop of each; then the wall time of one whole DPM-Solver++ chain and one whole DDIM chain.  Random weights: "
                      "no sample-quality claim" % a.ddim_steps,
              "model": a.model, "latent": [a.frames, 4, a.input_size, a.input_size], "batch": B, "operands": "f16", "guided": False,
              "steps": a.steps, "evaluations": evals, "reps": a.reps, "device": torch.cuda.get_device_name(0),
              "arch": torch.cuda.get_device_properties(0).gcnArchName, "box": socket.gethostname(),
              "ms_per_evaluation": ms, "median_ms_per_evaluation": med,
              "fused_over_ddim_step": {k: med[k]["fused"] / med[k]["ddim"] for k in METHODS},
              "stepwise_over_fused": {k: med[k]["stepwise"] / med[k]["fused"] for k in METHODS},
              "spread_of_the_yardstick": (max(all_ddim) - min(all_ddim)) / statistics.median(all_ddim),
              "stepwise_vs_fused_rel_l2": {k: float((out["stepwise", k] - out["fused", k]).norm() / out["fused", k].norm()) for k in METHODS},
              "wall_ms": {"dpmsolver++_%d" % a.steps: wall_dpm, "ddim_%d" % n: wall_ddim, "ddim_over_dpmsolver++": wall_ddim / wall_dpm},
              "finite": bool(all(torch.isfinite(v).all() for v in out.values())),
              "ddim_chain_finite": bool(torch.isfinite(x).all())}     # (an untrained model's long chain may leave the fp32 range)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({k: result[k] for k in ("median_ms_per_evaluation", "fused_over_ddim_step", "stepwise_over_fused", "spread_of_the_yardstick",
                                             "stepwise_vs_fused_rel_l2", "wall_ms", "finite", "box")}))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
