"""fp32 restatement of known-region sampling (the replacement scheme of Video Diffusion Models / RePaint; the reference has no such
function): the DDPM / DDIM chain of ``oracle.diffusion_oracle`` (``p_sample``, ``ddim_sample``, ``Schedule``) with the known part of the
sample overwritten, after every step, by the known clip diffused to the level the step has just reached, optionally with every index
repeated (``resample``) behind a one-level forward jump.  ``oracle.latte_oracle`` is the denoiser, on fixture M of tests/bpd_reference.py
(a two-block class-conditional Latte, gates N(0, 0.1), B = 2, F = 4, 8 x 8 latents).

Noise is consumed in slabs, in the order ``latte_known_chain_slabs`` defines: the start blend; then per repetition the step's own noise
(DDPM at i > 0, DDIM where eta != 0 and i > 0), the blend's (i > 0), the jump's (u < resample and i > 0)."""
import numpy as np
import torch

import bpd_reference as br
from invert_reference import M_CFG_SCALE, one_thread
from oracle import diffusion_oracle as do
from oracle import latte_oracle as lo

M_SPEC = br.M_SPEC
SLAB_SEED = 23
START_SEED = 29

# name -> spacing, method, eta, clip_denoised, resample, guided, mask arguments (frames, box)
CASES = {
    "ddim_keyframes": dict(spec="50", method="ddim", eta=0.0, clip=True, resample=1, guided=False, frames=[0, 3], box=None),
    "ddpm_prefix": dict(spec="50", method="ddpm", eta=0.0, clip=True, resample=1, guided=False, frames=[0, 1], box=None),
    "ddpm_box_clip0": dict(spec="50", method="ddpm", eta=0.0, clip=False, resample=1, guided=False, frames=None, box=(2, 2, 6, 6)),
    "ddim_eta1_box": dict(spec="50", method="ddim", eta=1.0, clip=True, resample=1, guided=False, frames=None, box=(2, 2, 6, 6)),
    "guided": dict(spec="50", method="ddim", eta=0.0, clip=True, resample=1, guided=True, frames=[0], box=None),
    "ddpm_10x3": dict(spec="10", method="ddpm", eta=0.0, clip=True, resample=3, guided=False, frames=[0, 1], box=None),
}


def mask_of(shape, frames=None, box=None):
    """[B, F, H, W] fp32, 1 = known: whole frames and / or the latent-pixel box (y0, x0, y1, x1), written out independently of
    ``latte_amd.known_mask``."""
    B, F, _, H, W = shape
    m = torch.zeros(B, F, H, W)
    for f in frames or ():
        m[:, f] = 1.0
    if box is not None:
        m[:, :, box[0]:box[2], box[1]:box[3]] = 1.0
    return m


def level(abar):
    """fp32 (sqrt(abar), sqrt(1 - abar)) of a level."""
    ab = torch.tensor(abar, dtype=torch.float64).float()
    return torch.sqrt(ab), torch.sqrt(1 - ab)


def blend(x, known, mask, abar, z):
    """x with its known part replaced by ``known`` at level ``abar`` (z = None: the clean latents).  mask [B, F, H, W]."""
    m = mask[:, :, None]
    kn = known
    if z is not None:
        a, b = level(abar)
        kn = a * known + b * z
    return torch.where(m == 1, kn, torch.where(m == 0, x, m * kn + (1 - m) * x))


def step_draws(method, eta, i):
    return i > 0 and (method == "ddpm" or eta != 0.0)


def slab_count(n_hi, n_lo, method, eta, resample, blend_start):
    """Hand count of the slabs of indices n_hi ... n_lo (descending, inclusive)."""
    n = int(bool(blend_start))
    for i in range(n_hi, n_lo - 1, -1):
        per_rep = int(step_draws(method, eta, i)) + int(i > 0)
        n += resample * per_rep + (resample - 1) * int(i > 0)
    return n


def known_loop(s, model_fn, x, known, mask, slabs, method="ddim", eta=0.0, clip_denoised=True, resample=1, start=None, end=0,
               blend_start=True):
    """-> [x after the blend of the last repetition of every index, start ... end].  ``model_fn(x, t_original int64[N])``."""
    start = s.num_timesteps - 1 if start is None else start
    it = iter(slabs)
    if blend_start:
        x = blend(x, known, mask, s.alphas_cumprod[start], next(it))
    trail = []
    for i in range(start, end - 1, -1):
        t = torch.full((x.shape[0],), s.timestep_map[i], dtype=torch.int64)
        for u in range(1, resample + 1):
            out = model_fn(x, t)
            nz = next(it) if step_draws(method, eta, i) else None
            if method == "ddim":
                x = do.ddim_sample(s, out, x, i, nz, eta, clip_denoised)["sample"]
            else:
                x = do.p_sample(s, out, x, i, nz if nz is not None else torch.zeros_like(x), clip_denoised)["sample"]
            x = blend(x, known, mask, s.alphas_cumprod_prev[i], next(it) if i > 0 else None)
            if u < resample and i > 0:
                beta = do._coef(s.betas, i)
                x = torch.sqrt(1 - beta) * x + torch.sqrt(beta) * next(it)
        trail.append(x)
    assert next(it, None) is None, "the chain must consume every slab"
    return trail


def case_inputs(name):
    """-> dict(kw, cfg, sd, y, x_T, known, mask, slabs, schedule arguments...) of a case; the guided case on the doubled batch with
    null labels (sample.py:88-94), its x_T, known, mask and slabs doubled as the reference doubles z."""
    c = dict(CASES[name])
    kw, cfg, sd, x0, y, _ = br.model_inputs()
    s = do.Schedule(c["spec"])
    n = slab_count(s.num_timesteps - 1, 0, c["method"], c["eta"], c["resample"], True)
    g = torch.Generator("cpu").manual_seed(SLAB_SEED)
    slabs = torch.randn((n,) + tuple(x0.shape), generator=g)
    x_T = torch.randn(x0.shape, generator=torch.Generator("cpu").manual_seed(START_SEED))
    mask = mask_of(x0.shape, c["frames"], c["box"])
    known = x0
    if c["guided"]:
        x_T, known, mask = (torch.cat([v, v]) for v in (x_T, known, mask))
        slabs = torch.cat([slabs, slabs], dim=1)
        y = torch.cat([y, torch.full_like(y, cfg.num_classes)])
    c.update(kw=kw, cfg=cfg, sd=sd, y=y, x_T=x_T, known=known, mask=mask, slabs=slabs, s=s)
    return c


def model_fn_of(c, perturb=0.0):
    """The fp32 oracle denoiser of a case.  ``perturb``: every output gets rel * rms(output) * N(0, 1) added (a relative-L2
    perturbation of that size), from a fixed generator."""
    sd, cfg, y = c["sd"], c["cfg"], c["y"]
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


CHECKPOINTS = {"50": (0, 24, 48, 49), "10": (0, 4, 8, 9)}   # executed indices kept: three intermediate trail entries and the final sample
_CACHE = {}


def restatement(name, perturb=0.0):
    """The restated chain of a case -> [len(CHECKPOINTS), B, ...] fp32 at the case's checkpoints.  Computed once per session."""
    key = (name, perturb)
    if key not in _CACHE:
        c = case_inputs(name)
        with torch.no_grad(), one_thread():
            trail = known_loop(c["s"], model_fn_of(c, perturb), c["x_T"], c["known"], c["mask"], c["slabs"], c["method"], c["eta"],
                               c["clip"], c["resample"])
        _CACHE[key] = torch.stack([trail[k] for k in CHECKPOINTS[c["spec"]]])
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
