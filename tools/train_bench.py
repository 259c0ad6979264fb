"""Training-step throughput on the engine (BASELINE config 5: Latte-B/2 16x256x256 synthetic latents; per-GPU micro-batch as
configs/ffs/ffs_train.yaml's local_batch_size = 5).  Prints ms per step and algorithmic TFLOP/s (3 x forward FLOPs).
LATTE_TRAIN_ACCUM=A: gradient accumulation over A micro-batches; "ms_per_step" then is the time per MICRO-batch (A of them and one
optimiser step make a window; LATTE_TRAIN_STEPS counts windows).
LATTE_TRAIN_CUSTOM=1: the cost of the custom-loss path instead -- three arms in one process, interleaved, LATTE_TRAIN_RUNS (5) runs of
LATTE_TRAIN_STEPS steps each: the built-in step, train_step(loss_fn=) with the built-in loss (MSE + variational bound) written in
torch, and the same through LatteTrainer.forward with x_t.requires_grad (the input gradient on top).  Prints the medians, each
arm's spread and the ratios against the built-in step of the same process."""
import sys, os, time, json
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import latte_amd

name = os.environ.get("LATTE_TRAIN_MODEL", "Latte-B/2")
B = int(os.environ.get("LATTE_TRAIN_BATCH", "5"))
steps = int(os.environ.get("LATTE_TRAIN_STEPS", "10"))
dtype = os.environ.get("LATTE_TRAIN_DTYPE", "f16")
accum = int(os.environ.get("LATTE_TRAIN_ACCUM", "1"))
model = latte_amd.Latte_models[name](input_size=32, num_frames=16, extras=1, max_batch=B).to("cuda")
with torch.no_grad():
    for p in model.parameters():
        if p.requires_grad and float(p.abs().max()) == 0.0:
            p.normal_(0, 0.02)
kw = {"gradient_accumulation_steps": accum} if accum != 1 else {}
tr = latte_amd.LatteTrainer(model, latte_amd.create_diffusion(""), max_batch=B, compute_dtype=dtype, **kw)
for kv in os.environ.get("LATTE_TRAIN_OPTIONS", "").split(","):   # e.g. LATTE_TRAIN_OPTIONS=fuse_gelu=0
    if kv:
        k, v = kv.split("=")
        tr.set_option(k, float(v))
g = torch.Generator("cpu").manual_seed(0)
x = torch.randn(B, 16, 4, 32, 32, generator=g).cuda()


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
print(json.dumps({"model": name, "operands": dtype, "local_batch": B, "accum": accum, "ms_per_step": round(dt * 1e3, 3), "samples_per_s": round(B / dt, 2),
                  "algorithmic_tflops": round(3 * fwd / dt / 1e12, 1), "forward_gflop": round(fwd / 1e9, 1),
                  "loss": float(out["loss"].mean()), "grad_norm": float(out["grad_norm"])}))
