"""Side measurement: the guided text-to-video chain of every self-contained scheduler, inside the engine and step by step.

  python tools/t2v_scheduler_bench.py [--layers 28] [--reps 2] [--parity-log FILE] [--out profiles/t2v_schedulers.json]

Latte-1's shape (16 frames of a 64x64 latent, 120 text tokens, random weights).  For each of DDIM 50, EulerDiscrete 50,
EulerAncestralDiscrete 50, HeunDiscrete 25 and DPMSolverMultistep 20 steps: ms per chain of the fused run (latte_t2v_guided_ddim_loop /
latte_t2v_guided_linear_loop) and of the step-by-step loop around the engine denoiser, interleaved in one process, device events
around whole chains after a short warm-up chain of each; evaluations per chain; rel-L2 between the two runs' latents (same seed).
The events enclose the whole pipeline call, so EulerAncestralDiscrete's fused time includes its 50 noise draws on the CPU generator and
their uploads in front of the engine call (the step-by-step loop makes the same draws between its steps): read its ratio with that.
--parity-log: the -s output of tests/test_t2v_schedulers.py on the GPU; its printed parities (fused vs step-by-step on the tiny
fixture, engine chain vs oracle loop) are copied into the JSON beside the times."""
import argparse
import json
import os
import re
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import latte_amd  # noqa: E402
from latte_amd import schedulers  # noqa: E402
from latte_amd.random_init import t2v_state_dict  # noqa: E402

METHODS = [("DDIM", schedulers.DDIMScheduler, 50), ("EulerDiscrete", schedulers.EulerDiscreteScheduler, 50),
           ("EulerAncestralDiscrete", schedulers.EulerAncestralDiscreteScheduler, 50),
           ("HeunDiscrete", schedulers.HeunDiscreteScheduler, 25), ("DPMSolverMultistep", schedulers.DPMSolverMultistepScheduler, 20)]


def parse_parity_log(path):
    out = {"fused_vs_stepwise_tiny_fixture": {}, "engine_vs_oracle_loop": {}}
    for line in open(path):
        m = re.search(r"(\w+): fused chain vs step-by-step loop rel-L2 ([0-9.e+-]+)", line)
        if m:
            out["fused_vs_stepwise_tiny_fixture"][m.group(1)] = float(m.group(2))
        m = re.search(r"(\w+): engine chain vs oracle loop rel-L2 ([0-9.e+-]+)", line)
        if m:
            out["engine_vs_oracle_loop"][m.group(1)] = float(m.group(2))
        m = re.search(r"Euler vs DDIM pipeline latents rel-L2 ([0-9.e+-]+)", line)
        if m:
            out["euler_vs_ddim_pipeline"] = float(m.group(1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=28)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--guidance", type=float, default=7.5)
    ap.add_argument("--parity-log", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "t2v_schedulers.json"))
    a = ap.parse_args()
    torch.set_grad_enabled(False)
    m = latte_amd.LatteT2V(num_layers=a.layers, max_batch=2).load_state_dict(t2v_state_dict(0, num_layers=a.layers))
    pipe = latte_amd.LattePipeline(transformer=m, scheduler=schedulers.DDIMScheduler()).to("cuda")
    g = torch.Generator("cpu").manual_seed(0)
    pe, ne = torch.randn(1, 120, 4096, generator=g), torch.randn(1, 120, 4096, generator=g)
    lat = torch.randn(1, 4, 16, 64, 64, generator=g)

    def chain(cls, steps, fused):
        pipe.scheduler = cls()
        pipe.allow_fused_loop = fused
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        out = pipe(prompt_embeds=pe, negative_prompt_embeds=ne, num_inference_steps=steps, guidance_scale=a.guidance, latents=lat,
                   generator=torch.Generator("cpu").manual_seed(1), output_type="latents").video
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]), out, len(pipe.scheduler.timesteps)

    print("model ready, warm-up chains", flush=True)
    for _, cls, _ in METHODS:                     # warm-up: a 3-step chain of each method in both forms
        for fused in (True, False):
            chain(cls, 3, fused)
    rows = {name: {"steps": steps, "fused_ms": [], "stepwise_ms": []} for name, _, steps in METHODS}
    for _ in range(a.reps):
        for name, cls, steps in METHODS:          # interleaved: fused, step by step, next method
            ms_fused, out_fused, n_evals = chain(cls, steps, True)
            ms_step, out_step, _ = chain(cls, steps, False)
            r = rows[name]
            r["fused_ms"].append(ms_fused)
            r["stepwise_ms"].append(ms_step)
            r["evaluations"] = n_evals
            r["fused_vs_stepwise_rel_l2"] = float((out_fused.double() - out_step.double()).norm() / out_step.double().norm())
            r["finite"] = bool(torch.isfinite(out_fused).all())
            print(f"  {name}: fused {ms_fused:.1f} ms, step by step {ms_step:.1f} ms", flush=True)
    for name, r in rows.items():
        r["fused_ms_per_chain"] = min(r["fused_ms"])
        r["stepwise_ms_per_chain"] = min(r["stepwise_ms"])
        r["fused_ms_per_evaluation"] = r["fused_ms_per_chain"] / r["evaluations"]
        print(f"{name:24s} {r['steps']:3d} steps {r['evaluations']:3d} evals: fused {r['fused_ms_per_chain']:9.1f} ms, step by step "
              f"{r['stepwise_ms_per_chain']:9.1f} ms per chain ({r['stepwise_ms_per_chain'] / r['fused_ms_per_chain']:.4f} x), "
              f"rel-L2 {r['fused_vs_stepwise_rel_l2']:.2e}, finite={r['finite']}")
    result = {"what": "guided text-to-video chains at Latte-1's shape (16 x 64 x 64 latents, 120 text tokens, random weights), ms per chain "
                      "from device events around whole chains, best of `reps` interleaved repetitions after a 3-step warm-up chain",
              "layers": a.layers, "reps": a.reps, "guidance_scale": a.guidance, "device": torch.cuda.get_device_name(0),
              "methods": rows,
              "test_parities": parse_parity_log(a.parity_log) if a.parity_log else "not measured"}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
