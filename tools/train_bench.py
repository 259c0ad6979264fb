"""Training-step throughput on the engine (BASELINE config 5: Latte-B/2 16x256x256 synthetic latents; per-GPU micro-batch as
configs/ffs/ffs_train.yaml's local_batch_size = 5).  Prints ms per step and algorithmic TFLOP/s (3 x forward FLOPs).
LATTE_TRAIN_ACCUM=A: gradient accumulation over A micro-batches; "ms_per_step" then is the time per MICRO-batch (A of them and one
optimiser step make a window; LATTE_TRAIN_STEPS counts windows).
LATTE_TRAIN_CUSTOM=1: the cost of the custom-loss path instead -- three arms in one process, interleaved, LATTE_TRAIN_RUNS (5) runs of
LATTE_TRAIN_STEPS steps each: the built-in step, train_step(loss_fn=) with the built-in loss (MSE + variational bound) written in
torch, and the same through LatteTrainer.forward with x_t.requires_grad (the input gradient on top).  Prints the medians, each
arm's spread and the ratios against the built-in step of the same process.
--lora-rank R (or LATTE_TRAIN_LORA_RANK=R): the LoRA step (LatteTrainer(lora_rank=R), all four targets) instead of the full one.
LATTE_TRAIN_LORA_AB=16,32: the full step against the LoRA step at those ranks -- one trainer per arm in one process, interleaved,
LATTE_TRAIN_RUNS (5) runs of LATTE_TRAIN_STEPS steps each; prints the medians, each arm's spread, the speed-ups, the adapter file size
and the device memory each trainer took."""
import sys, os, time, json
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import latte_amd

name = os.environ.get("LATTE_TRAIN_MODEL", "Latte-B/2")
B = int(os.environ.get("LATTE_TRAIN_BATCH", "5"))
steps = int(os.environ.get("LATTE_TRAIN_STEPS", "10"))
dtype = os.environ.get("LATTE_TRAIN_DTYPE", "f16")
accum = int(os.environ.get("LATTE_TRAIN_ACCUM", "1"))
lora_rank = int(os.environ.get("LATTE_TRAIN_LORA_RANK", "0"))
if "--lora-rank" in sys.argv:
    lora_rank = int(sys.argv[sys.argv.index("--lora-rank") + 1])


def make_trainer(rank=0, **kw):
    model = latte_amd.Latte_models[name](input_size=32, num_frames=16, extras=1, max_batch=B).to("cuda")
    with torch.no_grad():
        gen = torch.Generator("cuda").manual_seed(1)
        for p in model.parameters():
            if p.requires_grad and float(p.abs().max()) == 0.0:
                p.normal_(0, 0.02, generator=gen)
    if rank:
        kw["lora_rank"] = rank
    return model, latte_amd.LatteTrainer(model, latte_amd.create_diffusion(""), max_batch=B, compute_dtype=dtype, **kw)


def lora_ab(ranks):
    import statistics
    runs = int(os.environ.get("LATTE_TRAIN_RUNS", "5"))
    arms, mem = {}, {}
    for key, r in [("full", 0)] + [(f"lora{r}", r) for r in ranks]:
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        free0 = torch.cuda.mem_get_info()[0]
        arms[key] = make_trainer(r)[1]
        torch.cuda.synchronize()
        # torch's buffers (parameters, gradients, moments, EMA / adapters) and everything the engine allocated itself
        mem[key] = {"torch_mb": round((torch.cuda.memory_allocated() - before) / 2 ** 20, 1),
                    "device_mb": round((free0 - torch.cuda.mem_get_info()[0]) / 2 ** 20, 1)}
    for tr_ in arms.values():
        for _ in range(3):
            tr_.train_step(x)
    ms = {k: [] for k in arms}
    for _ in range(runs):
        for k, tr_ in arms.items():
            torch.cuda.synchronize()
            t0 = time.time()
            for _ in range(steps):
                out_ = tr_.train_step(x)
            torch.cuda.synchronize()
            ms[k].append((time.time() - t0) / steps * 1e3)
    med = {k: statistics.median(v) for k, v in ms.items()}
    print(json.dumps({"model": name, "operands": dtype, "local_batch": B, "steps_per_run": steps, "runs": runs,
                      "ms_per_step": {k: round(v, 3) for k, v in med.items()},
                      "ms_per_step_runs": {k: [round(x_, 3) for x_ in v] for k, v in ms.items()},
                      "spread": {k: round((max(v) - min(v)) / med[k], 4) for k, v in ms.items()},
                      "speedup": {k: round(med["full"] / med[k], 4) for k in med if k != "full"},
                      "adapter_file_mb": {k: round(arms[k].lora_params.numel() * 4 / 2 ** 20, 2) for k in arms if k != "full"},
                      "memory": mem}))


kw = {"gradient_accumulation_steps": accum} if accum != 1 else {}
g = torch.Generator("cpu").manual_seed(0)
x = torch.randn(B, 16, 4, 32, 32, generator=g).cuda()
if os.environ.get("LATTE_TRAIN_LORA_AB"):
    lora_ab([int(r) for r in os.environ["LATTE_TRAIN_LORA_AB"].split(",")])
    sys.exit(0)
model, tr = make_trainer(lora_rank, **kw)
for kv in os.environ.get("LATTE_TRAIN_OPTIONS", "").split(","):   # e.g. LATTE_TRAIN_OPTIONS=fuse_gelu=0
    if kv:
        k, v = kv.split("=")
        tr.set_option(k, float(v))


def custom_arms():
    import math
    import statistics
    d = tr.diffusion
    tab = {k: torch.tensor(getattr(d, k), dtype=torch.float32, device="cuda") for k in
           ("posterior_mean_coef1", "posterior_mean_coef2", "posterior_log_variance_clipped", "log_betas", "sqrt_recip_alphas_cumprod",
            "sqrt_recipm1_alphas_cumprod")}

    def cdf(v):
        return 0.5 * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (v + 0.044715 * v ** 3)))

    def builtin_in_torch(out, x_start, x_t, t, noise):
        """training_losses' "mse" + "vb" (gaussian_diffusion.py:743-787): the bound sees the mean head detached."""
        c = {k: v[t].view(-1, 1, 1, 1, 1) for k, v in tab.items()}
        eps, v = out[:, :, :4], out[:, :, 4:]
        mse = ((noise - eps) ** 2).flatten(1).mean(1)
        e = eps.detach()
        frac = (v + 1) / 2
        logvar = frac * c["log_betas"] + (1 - frac) * c["posterior_log_variance_clipped"]
        x0 = c["sqrt_recip_alphas_cumprod"] * x_t - c["sqrt_recipm1_alphas_cumprod"] * e
        mean = c["posterior_mean_coef1"] * x0 + c["posterior_mean_coef2"] * x_t
        true_mean = c["posterior_mean_coef1"] * x_start + c["posterior_mean_coef2"] * x_t
        lv1 = c["posterior_log_variance_clipped"]
        kl = 0.5 * (-1.0 + logvar - lv1 + torch.exp(lv1 - logvar) + (true_mean - mean) ** 2 * torch.exp(-logvar))
        inv = torch.exp(-0.5 * logvar)
        cp, cm = cdf(inv * (x_start - mean + 1.0 / 255.0)), cdf(inv * (x_start - mean - 1.0 / 255.0))
        ll = torch.where(x_start < -0.999, torch.log(cp.clamp(min=1e-12)),
                         torch.where(x_start > 0.999, torch.log((1.0 - cm).clamp(min=1e-12)), torch.log((cp - cm).clamp(min=1e-12))))
        vb = torch.where(t == 0, (-ll).flatten(1).mean(1), kl.flatten(1).mean(1)) / math.log(2.0)
        return mse + vb

    tg = torch.Generator("cpu").manual_seed(1)
    ts = [torch.randint(0, d.num_timesteps, (B,), generator=tg).cuda() for _ in range(steps)]
    nz = torch.randn(B, 16, 4, 32, 32, generator=tg).cuda()

    def builtin(i):
        return tr.train_step(x, t=ts[i], noise=nz)["loss"]

    def custom(i):
        return tr.train_step(x, t=ts[i], noise=nz, loss_fn=builtin_in_torch)["loss"]

    def custom_dx(i):
        x_t = d.q_sample(x, ts[i], nz).requires_grad_(True)
        per = builtin_in_torch(tr.forward(x_t, ts[i]), x, x_t, ts[i], nz)       # create_diffusion(""): timestep_map is the identity
        per.mean().backward()
        tr.optimizer_step()
        assert x_t.grad is not None
        return per.detach()

    arms = {"builtin": builtin, "custom": custom, "custom_dx": custom_dx}
    runs = int(os.environ.get("LATTE_TRAIN_RUNS", "5"))
    ms = {k: [] for k in arms}
    loss = {}
    for r in range(runs + 1):                                # run 0 warms every arm up
        for k, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.time()
            for i in range(steps):
                out = fn(i)
            torch.cuda.synchronize()
            if r:
                ms[k].append((time.time() - t0) / steps * 1e3)
            loss[k] = float(out.mean())
    med = {k: statistics.median(v) for k, v in ms.items()}
    print(json.dumps({"model": name, "operands": dtype, "local_batch": B, "steps_per_run": steps, "runs": runs,
                      "ms_per_step_median": {k: round(v, 3) for k, v in med.items()},
                      "ms_per_step_runs": {k: [round(x_, 3) for x_ in v] for k, v in ms.items()},
                      "spread": {k: round((max(v) - min(v)) / med[k], 4) for k, v in ms.items()},
                      "ratio_custom": round(med["custom"] / med["builtin"], 4), "ratio_custom_dx": round(med["custom_dx"] / med["builtin"], 4),
                      "last_loss": loss}))


if os.environ.get("LATTE_TRAIN_CUSTOM"):
    custom_arms()
    sys.exit(0)
for _ in range(2 * accum):
    out = tr.train_step(x)
torch.cuda.synchronize()
t0 = time.time()
for _ in range(steps * accum):
    out = tr.train_step(x)
torch.cuda.synchronize()
dt = (time.time() - t0) / (steps * accum)
D, depth, Hm = model.hidden_size, model.depth, model.mlp_hidden
M = B * 16 * 256
lin = depth * 2.0 * M * (4 * D * D + 2 * D * Hm)
attn = (depth // 2) * (4.0 * B * 16 * 256 * 256 * D + 4.0 * B * 256 * 16 * 16 * D)
fwd = lin + attn
print(json.dumps({"model": name, "operands": dtype, "local_batch": B, "accum": accum, "lora_rank": lora_rank, "ms_per_step": round(dt * 1e3, 3), "samples_per_s": round(B / dt, 2),
                  "algorithmic_tflops": round(3 * fwd / dt / 1e12, 1), "forward_gflop": round(fwd / 1e9, 1),
                  "loss": float(out["loss"].mean()), "grad_norm": float(out["grad_norm"])}))
