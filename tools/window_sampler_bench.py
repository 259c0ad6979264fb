"""Side measurement: per-step time of sampling a long clip with overlapping temporal windows against the unchanged loops on the same
number of clips, at the headline shape.

  python tools/window_sampler_bench.py [--model Latte-XL/2] [--samples 2] [--total-frames 40] [--stride 8] [--steps 20] [--reps 5]
                                       [--out profiles/window_sampler.json] [--bench-line FILE --parent-bench-line FILE]

Latte-XL/2, 16 frames of 32x32 latents, f16 operands, random weights.  N = 2 clips of L = 40 frames at stride 8: 4 windows, 8 clips per
denoiser evaluation.  The yardstick is the unchanged loop at B = 8 -- the same forward.  Interleaved in one process, device events
around each whole loop, medians of `reps` repetitions after one warm-up loop of each:
  ddim         create_diffusion("250"), `steps` respaced indices (249 ... 250 - steps), DDIM eta 0:
    window       ONE latte_sample_loop_windows call on [2, 40, 4, 32, 32]
    plain        SpacedDiffusion.ddim_sample_loop on [8, 16, 4, 32, 32]: ONE latte_sample_loop_ex call
  dpmsolver++  create_diffusion("20"), the whole chain of 20 evaluations:
    window       SpacedDiffusion.window_sample_loop(method="dpmsolver++"): ONE latte_sample_plan_loop_windows call
    plain        SpacedDiffusion.linear_sample_loop at B = 8: ONE latte_sample_plan_loop call
A windowed step is the plain step plus two launches (gather: 2.6 MB read and written; merge: 5.2 MB read, 3.3 MB written) and the
update over 10 latent frames per clip row instead of 16: under 0.1 % of a 30 ms step either way, so the ratio is expected at 1 within
the spread of the interleaved repeats.  Rule: the ratio of the medians lies inside the yardstick's own min ... max (over its median),
widened once by that spread.  --bench-line / --parent-bench-line: files holding the JSON result line of a default
``bench.py --gpus 1`` run on this commit and on its parent; both are recorded in the output.  The box is named in the file."""
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


def last_json_line(path):
    with open(path) as f:
        lines = [ln for ln in f.read().splitlines() if ln.strip().startswith("{")]
    return json.loads(lines[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="Latte-XL/2")
    ap.add_argument("--samples", type=int, default=2)
    ap.add_argument("--total-frames", type=int, default=40)
    ap.add_argument("--stride", type=int, default=8)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--input-size", type=int, default=32)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--bench-line", default="")
    ap.add_argument("--parent-bench-line", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "window_sampler.json"))
    a = ap.parse_args()
    torch.set_grad_enabled(False)
    if not torch.cuda.is_available():
        raise SystemExit("tools/window_sampler_bench.py needs an MI355X")
    N, L, F, S = a.samples, a.total_frames, a.frames, a.stride
    starts = latte_amd.window_starts(L, F, S)
    W = len(starts)
    B = N * W
    m = latte_amd.Latte_models[a.model](input_size=a.input_size, num_frames=F, num_classes=101, extras=2, learn_sigma=True,
                                        compute_dtype="f16", max_batch=B)
    g = torch.Generator("cpu").manual_seed(1)
    for _, p in m.named_parameters():        # the zero-initialised gates and final layer re-drawn: every block reaches the output
        if p.requires_grad and float(p.detach().abs().max()) == 0.0:
            p.copy_(torch.randn(p.shape, generator=g) * 0.02)
    m = m.cuda().eval()
    lib = load_library()
    d250, d20 = latte_amd.create_diffusion("250"), latte_amd.create_diffusion("20")
    hi, lo = d250.num_timesteps - 1, d250.num_timesteps - a.steps
    long_shape, clip_shape = (N, L, 4, a.input_size, a.input_size), (B, F, 4, a.input_size, a.input_size)
    z_long, z_clip = torch.randn(long_shape, generator=g).cuda(), torch.randn(clip_shape, generator=g).cuda()
    y_long, y_clip = torch.randint(0, 101, (N,), generator=g).cuda(), torch.randint(0, 101, (B,), generator=g).cuda()
    out = {}

    def ddim_window():
        ec = d250._engine_chain(m.forward, z_long.clone(), dict(y=y_long), windows=W)
        check(lib.latte_sample_loop_windows(ec.eng, d250._h, 1, 0.0, 0, 0, 1.0, ptr(ec.x32), ptr(ec.y64), N, hi, lo, None, None, None, L, S,
                                            stream_ptr()))
        out["ddim_window"] = ec.x32

    def ddim_plain():
        out["ddim_plain"] = d250.ddim_sample_loop(m.forward, clip_shape, z_clip, clip_denoised=False, model_kwargs=dict(y=y_clip),
                                                  start_index=hi, end_index=lo)

    def dpm_window():
        out["dpm_window"] = d20.window_sample_loop(m.forward, long_shape, z_long, method="dpmsolver++", stride=S, model_kwargs=dict(y=y_long))

    def dpm_plain():
        out["dpm_plain"] = d20.linear_sample_loop(m.forward, clip_shape, z_clip, method="dpmsolver++", model_kwargs=dict(y=y_clip))

    loops = {"ddim_window": (ddim_window, a.steps), "ddim_plain": (ddim_plain, a.steps), "dpm_window": (dpm_window, d20.num_timesteps),
             "dpm_plain": (dpm_plain, d20.num_timesteps)}

    def timed(fn, steps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / steps

    print("model ready, warm-up", flush=True)
    for fn, steps in loops.values():
        timed(fn, steps)
    ms = {k: [] for k in loops}
    for r in range(a.reps):
        for k, (fn, steps) in loops.items():          # interleaved
            ms[k].append(timed(fn, steps))
        print("  rep %d: " % r + ", ".join("%s %.3f" % (k, v[-1]) for k, v in ms.items()) + " ms per step", flush=True)
    med = {k: statistics.median(v) for k, v in ms.items()}

    def verdict(win, plain):
        ratio = med[win] / med[plain]
        lo_, hi_ = min(ms[plain]) / med[plain], max(ms[plain]) / med[plain]
        spread = hi_ - lo_
        return {"window_step_over_plain_step": ratio, "ratio_per_repetition": [w_ / p_ for w_, p_ in zip(ms[win], ms[plain])],
                "yardstick_min_max_over_median": [lo_, hi_], "spread_of_the_yardstick": spread,
                "spread_of_the_window_chain": (max(ms[win]) - min(ms[win])) / med[win],
                "inside_the_widened_range": bool(lo_ - spread <= ratio <= hi_ + spread)}

    result = {"what": "ms per step of sampling N clips of L frames with overlapping temporal windows (W windows, N W clips per evaluation) as "
                      "one latte_sample_loop_windows / latte_sample_plan_loop_windows call, and of the unchanged ddim_sample_loop / "
                      "linear_sample_loop at B = N W; device events around whole loops, medians of `reps` interleaved repetitions after "
                      "one warm-up loop of each",
              "model": a.model, "clip": [F, 4, a.input_size, a.input_size], "samples": N, "total_frames": L, "stride": S, "window_starts": starts,
              "clips_per_evaluation": B, "operands": "f16", "ddim_steps_per_loop": a.steps, "dpm_evaluations_per_loop": d20.num_timesteps,
              "reps": a.reps, "device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName,
              "box": socket.gethostname(), "ms_per_step": ms, "median_ms_per_step": med,
              "ddim": verdict("ddim_window", "ddim_plain"), "dpmsolver++": verdict("dpm_window", "dpm_plain"),
              "finite": bool(all(torch.isfinite(v).all() for v in out.values()))}
    if a.bench_line:
        result["bench_this_commit"] = last_json_line(a.bench_line)
    if a.parent_bench_line:
        result["bench_parent_commit"] = last_json_line(a.parent_bench_line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"median_ms_per_step": med, "ddim": result["ddim"]["window_step_over_plain_step"],
                      "ddim_inside": result["ddim"]["inside_the_widened_range"], "dpmsolver++": result["dpmsolver++"]["window_step_over_plain_step"],
                      "dpm_inside": result["dpmsolver++"]["inside_the_widened_range"], "finite": result["finite"], "box": result["box"]}))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
