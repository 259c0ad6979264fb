"""fp32 restatement of sampling a clip longer than ``num_frames`` with overlapping temporal windows (temporal co-denoising as in
Gen-L-Video / MultiDiffusion along time; the reference has no such function): at every denoiser evaluation the model runs on the
F-frame windows of the long latent, the outputs are averaged with uniform weights where windows overlap, and one ordinary step is
applied to the long latent.  The DDPM / DDIM steps are ``oracle.diffusion_oracle`` (``p_sample``, ``ddim_sample``, ``Schedule``); the
linear samplers ("dpmsolver++", "heun") are the host schedulers of ``latte_amd.schedulers`` on the diffusion's own timesteps, which
tests/test_linear_sampler.py ties to the DDIM recursion; ``oracle.latte_oracle`` is the denoiser, on fixture M of
tests/bpd_reference.py (a two-block class-conditional Latte, gates N(0, 0.1), B = 2, F = 4, 8 x 8 latents).

The window set is written out here independently of ``latte_window_plan``:
    W = ceil((L - F) / stride) + 1,   s_w = min(w * stride, L - F)
Clip ``g * W + w`` is window w of batch row g; labels are repeated per window; the merge sums in ascending w and divides by the count.

Noise: row k is read at the k-th executed step (DDPM at i > 0, DDIM where eta != 0 and i > 0)."""
import torch

import bpd_reference as br
from invert_reference import M_CFG_SCALE, one_thread
from known_reference import CHECKPOINTS  # noqa: F401  (the executed indices the tests compare at)
from oracle import diffusion_oracle as do
from oracle import latte_oracle as lo

NOISE_SEED = 23
START_SEED = 29
LINEAR = ("dpmsolver++", "heun")

# name -> spacing, method, eta, clip_denoised, guided, total frames L, stride
CASES = {
    "ddim_L10_s3": dict(spec="50", method="ddim", eta=0.0, clip=True, guided=False, L=10, stride=3),
    "ddpm_L9_s3_tail": dict(spec="50", method="ddpm", eta=0.0, clip=True, guided=False, L=9, stride=3),
    "ddim_eta1_L7_s2_clip0": dict(spec="50", method="ddim", eta=1.0, clip=False, guided=False, L=7, stride=2),
    "guided_L6_s2": dict(spec="50", method="ddim", eta=0.0, clip=True, guided=True, L=6, stride=2),
    "ddpm10_L8_s1": dict(spec="10", method="ddpm", eta=0.0, clip=True, guided=False, L=8, stride=1),
    "dpm10_L7_s2": dict(spec="10", method="dpmsolver++", eta=0.0, clip=False, guided=False, L=7, stride=2),
    "heun10_L6_s2": dict(spec="10", method="heun", eta=0.0, clip=False, guided=True, L=6, stride=2),
}
STARTS = {"ddim_L10_s3": [0, 3, 6], "ddpm_L9_s3_tail": [0, 3, 5], "ddim_eta1_L7_s2_clip0": [0, 2, 3], "guided_L6_s2": [0, 2],
          "ddpm10_L8_s1": [0, 1, 2, 3, 4], "dpm10_L7_s2": [0, 2, 3], "heun10_L6_s2": [0, 2]}


def starts_of(L, F, stride):
    assert L >= F and 1 <= stride <= F
    W = -(-(L - F) // stride) + 1
    return [min(w * stride, L - F) for w in range(W)]


def gather(x, F, starts):
    """[G, L, ...] -> [G * W, F, ...], clip g * W + w = x[g, s_w : s_w + F]."""
    return torch.stack([x[g, s:s + F] for g in range(x.shape[0]) for s in starts])


def merge(out, L, starts):
    """[G * W, F, ...] -> [G, L, ...]: per frame the fp32 sum over the covering windows in ascending w, divided by their count; a frame
    one window covers is copied."""
    W, F = len(starts), out.shape[1]
    G = out.shape[0] // W
    rows = []
    for g in range(G):
        frames = []
        for f in range(L):
            acc, n = None, 0
            for w, s in enumerate(starts):
                if s <= f < s + F:
                    v = out[g * W + w, f - s]
                    acc = v if acc is None else acc + v
                    n += 1
            frames.append(acc if n == 1 else acc / n)
        rows.append(torch.stack(frames))
    return torch.stack(rows)


def windowed(model_fn, F, L, starts):
    """The denoiser of the long latent: ``model_fn(clips, t int64[G * W])`` on the gathered clips, merged."""
    def fn(x, t):
        return merge(model_fn(gather(x, F, starts), t.repeat_interleave(len(starts))), L, starts)
    return fn


def step_draws(method, eta, i):
    return i > 0 and (method == "ddpm" or eta != 0.0)


def window_loop(s, fn, x, noise, method="ddim", eta=0.0, clip_denoised=True):
    """-> [x after every index, T - 1 ... 0].  ``fn(x, t_original int64[G])`` is the windowed denoiser."""
    trail = []
    for k, i in enumerate(range(s.num_timesteps - 1, -1, -1)):
        t = torch.full((x.shape[0],), s.timestep_map[i], dtype=torch.int64)
        out = fn(x, t)
        nz = noise[k] if step_draws(method, eta, i) else None
        if method == "ddim":
            x = do.ddim_sample(s, out, x, i, nz, eta, clip_denoised)["sample"]
        else:
            x = do.p_sample(s, out, x, i, nz if nz is not None else torch.zeros_like(x), clip_denoised)["sample"]
        trail.append(x)
    return trail


def linear_loop(sch, fn, x, C):
    """-> [x after every denoiser evaluation]: the scheduler's own scale_model_input / step around the windowed denoiser; the
    learned-sigma half of the output is dropped."""
    trail = []
    x = x * float(sch.init_noise_sigma)
    for t in sch.timesteps:
        out = fn(sch.scale_model_input(x, t), torch.full((x.shape[0],), int(t), dtype=torch.int64))
        x = sch.step(out[:, :, :C], t, x, return_dict=False)[0]
        trail.append(x)
    return trail


def case_inputs(name):
    """-> the case with kw, cfg, sd, y, x_T [G, L, C, H, W], noise [T, G, L, C, H, W], s, starts; the guided cases on the doubled
    batch with null labels (sample.py:88-94), x_T and the noise doubled as the reference doubles z."""
    c = dict(CASES[name])
    kw, cfg, sd, x0, y, _ = br.model_inputs()
    s = do.Schedule(c["spec"])
    shape = (x0.shape[0], c["L"]) + tuple(x0.shape[2:])
    noise = torch.randn((s.num_timesteps,) + shape, generator=torch.Generator("cpu").manual_seed(NOISE_SEED))
    x_T = torch.randn(shape, generator=torch.Generator("cpu").manual_seed(START_SEED))
    if c["guided"]:
        x_T = torch.cat([x_T, x_T])
        noise = torch.cat([noise, noise], dim=1)
        y = torch.cat([y, torch.full_like(y, cfg.num_classes)])
    starts = starts_of(c["L"], cfg.num_frames, c["stride"])
    assert starts == STARTS[name], (name, starts)
    c.update(kw=kw, cfg=cfg, sd=sd, y=y, x_T=x_T, noise=noise, s=s, starts=starts, F=cfg.num_frames)
    return c


def model_fn_of(c, perturb=0.0):
    """The fp32 oracle denoiser of a case ON THE CLIPS (labels repeated per window).  ``perturb``: every output gets
    rel * rms(output) * N(0, 1) added (a relative-L2 perturbation of that size), from a fixed generator."""
    sd, cfg = c["sd"], c["cfg"]
    y = c["y"].repeat_interleave(len(c["starts"]))
    if c["guided"]:
        fn = lambda xx, t: lo.latte_forward_with_cfg(sd, cfg, xx, t, y, M_CFG_SCALE)
    else:
        fn = lambda xx, t: lo.latte_forward(sd, cfg, xx, t, y)
    if not perturb:
        return fn
    g = torch.Generator("cpu").manual_seed(5)

    def noisy(xx, t):
        out = fn(xx, t)
        return out + perturb * out.pow(2).mean().sqrt() * torch.randn(out.shape, generator=g)
    return noisy


def linear_scheduler(c):
    import latte_amd
    return latte_amd.create_diffusion(c["spec"]).linear_scheduler(c["method"])


_CACHE = {}


def restatement(name, perturb=0.0):
    """The restated chain of a case -> [steps or evaluations, G, L, C, H, W] fp32, x after every one.  Computed once per session."""
    key = (name, perturb)
    if key not in _CACHE:
        c = case_inputs(name)
        fn = windowed(model_fn_of(c, perturb), c["F"], c["L"], c["starts"])
        with torch.no_grad(), one_thread():
            if c["method"] in LINEAR:
                trail = linear_loop(linear_scheduler(c), fn, c["x_T"], c["cfg"].in_channels)
            else:
                trail = window_loop(c["s"], fn, c["x_T"], c["noise"], c["method"], c["eta"], c["clip"])
        _CACHE[key] = torch.stack(trail)
    return _CACHE[key]


def growth(name, rel=3e-4):
    """Relative L2 by which a ``rel`` perturbation of every model output moves the restated chain's final sample."""
    a, b = restatement(name), restatement(name, rel)
    return float((a[-1] - b[-1]).double().norm() / a[-1].double().norm())


if __name__ == "__main__":
    import time
    for nm in CASES:
        t0 = time.time()
        restatement(nm)
        t1 = time.time()
        print(nm, f"restated in {t1 - t0:.2f} s; a 3e-4 perturbation moves it by {growth(nm):.2e}")
