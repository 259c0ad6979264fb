"""fp32 restatement of likelihood evaluation: ``GaussianDiffusion.calc_bpd_loop`` (gaussian_diffusion.py:813-866) with
``_vb_terms_bpd`` (:686-717, WITH ``clip_denoised``) and ``_prior_bpd`` (:797-811), plus the builders of the fixtures
tests/golden/bpd.npz is computed on (tools/make_bpd_golden.py).

Composed from the pinned CPU oracle (``oracle.diffusion_oracle``: ``p_mean_variance(clip_denoised=...)``, ``normal_kl``,
``discretized_gaussian_log_likelihood``, ``q_sample``, ``Schedule``).  tests/test_bpd_reference.py pins it to the committed fixture
-- what the reference objects computed -- and, where the reference is present, to the live reference.

Fixture M (model level): a two-block class-conditional Latte with gates drawn N(0, 0.1), B = 2, create_diffusion("50").
Fixtures K (kernel level): model outputs from ``synthetic_model`` for every ModelMeanType x ModelVarType create_diffusion builds,
three sample sizes, the first / second / middle / last index, ``clip_denoised`` on and off."""
import json
import os

import numpy as np
import torch

from oracle import diffusion_oracle as do
from oracle import latte_oracle as lo

# ---------------------------------------------------------------------------- the restatement
LN2 = np.log(2.0)


def prior_bpd(s, x_start):
    """gd:797-811: KL(q(x_T | x_0) || N(0, I)) in bits per dimension."""
    last = s.num_timesteps - 1
    qt_mean = do._coef(s.sqrt_alphas_cumprod, last) * x_start                     # gd:210
    qt_logvar = do._coef(np.log(1.0 - s.alphas_cumprod), last)                    # gd:183,212
    zero = torch.tensor(0.0)
    return do._mean_flat(do.normal_kl(qt_mean, qt_logvar, zero, zero)) / LN2


def bpd_terms(s, model_out, x_start, x_t, noise, i, clip_denoised):
    """One column of calc_bpd_loop (gd:839-852) for respaced index ``i`` -> (vb [N], xstart_mse [N], mse [N], pred_xstart)."""
    true_mean = do._coef(s.posterior_mean_coef1, i) * x_start + do._coef(s.posterior_mean_coef2, i) * x_t   # gd:232-241
    true_logvar = do._coef(s.posterior_log_variance_clipped, i)
    out = do.p_mean_variance(s, model_out, x_t, i, clip_denoised=clip_denoised)
    if i == 0:                                                                    # gd:708-716
        vb = do._mean_flat(-do.discretized_gaussian_log_likelihood(x_start, out["mean"], 0.5 * out["log_variance"])) / LN2
    else:
        vb = do._mean_flat(do.normal_kl(true_mean, true_logvar, out["mean"], out["log_variance"])) / LN2
    x0p = out["pred_xstart"]
    xstart_mse = do._mean_flat((x0p - x_start) ** 2)                              # gd:850
    eps = (do._coef(s.sqrt_recip_alphas_cumprod, i) * x_t - x0p) / do._coef(s.sqrt_recipm1_alphas_cumprod, i)   # gd:345-348
    return vb, xstart_mse, do._mean_flat((eps - noise) ** 2), x0p                 # gd:852


def calc_bpd_loop(s, model_fn, x_start, noises, clip_denoised=True):
    """gd:813-866.  ``model_fn(x_t, t_original int64[N])``; ``noises[k]`` is the draw of the k-th executed step (t = T-1 first)."""
    B = x_start.shape[0]
    cols = []
    for k, i in enumerate(range(s.num_timesteps - 1, -1, -1)):
        t = torch.full((B,), i, dtype=torch.int64)
        x_t = do.q_sample(s, x_start, t, noises[k])
        out = model_fn(x_t, torch.full((B,), s.timestep_map[i], dtype=torch.int64))
        cols.append(bpd_terms(s, out, x_start, x_t, noises[k], i, clip_denoised)[:3])
    vb, xstart_mse, mse = (torch.stack([c[j] for c in cols], dim=1) for j in range(3))
    prior = prior_bpd(s, x_start)
    return {"total_bpd": vb.sum(dim=1) + prior, "prior_bpd": prior, "vb": vb, "xstart_mse": xstart_mse, "mse": mse}


TABLES = ("total_bpd", "prior_bpd", "vb", "xstart_mse", "mse")


# ---------------------------------------------------------------------------- fixture M
M_MODEL = dict(depth=2, hidden_size=128, patch_size=2, num_heads=2, input_size=8, num_frames=4, num_classes=5, extras=2, learn_sigma=True)
M_SPEC = "50"
M_NOISE_SEED = 11


def model_inputs(extras=2, learn_sigma=True, spec=M_SPEC):
    """-> kw (ctor arguments), cfg, sd, x0 [2, F, C, H, W], y | None, noise [T, 2, F, C, H, W].  The noise is what T successive
    ``torch.randn_like(x0)`` give after ``torch.manual_seed(M_NOISE_SEED)``: the draws of the reference's own loop (gd:837)."""
    kw = dict(M_MODEL, extras=extras, learn_sigma=learn_sigma)
    cfg = lo.LatteConfig(**kw)
    sd = lo.init_state_dict(cfg, seed=3, gate_std=0.1)
    g = torch.Generator("cpu").manual_seed(31)
    x0 = (torch.randn(2, cfg.num_frames, cfg.in_channels, cfg.input_size, cfg.input_size, generator=g) * 0.6).clamp(-1.0, 1.0)
    y = torch.tensor([1, 3], dtype=torch.int64) if extras == 2 else None
    n = do.Schedule(spec).num_timesteps
    state = torch.random.get_rng_state()
    torch.manual_seed(M_NOISE_SEED)
    noise = torch.stack([torch.randn_like(x0) for _ in range(n)])
    torch.random.set_rng_state(state)
    return kw, cfg, sd, x0, y, noise


def model_restatement(extras=2, learn_sigma=True, clip_denoised=True, spec=M_SPEC):
    """The restatement on fixture M (or its unconditional / fixed-variance variant) with the fp32 oracle as the denoiser."""
    kw, cfg, sd, x0, y, noise = model_inputs(extras, learn_sigma, spec)
    s = do.Schedule(spec, learn_sigma=learn_sigma)
    with torch.no_grad():
        return calc_bpd_loop(s, lambda x, t: lo.latte_forward(sd, cfg, x, t, y), x0, noise, clip_denoised)


# ---------------------------------------------------------------------------- fixtures K
K_TYPES = {   # every ModelMeanType x ModelVarType create_diffusion builds (diffusion/__init__.py:32-45)
    "eps_learned": dict(),
    "eps_fixed_large": dict(learn_sigma=False),
    "eps_fixed_small": dict(learn_sigma=False, sigma_small=True),
    "xstart_learned": dict(predict_xstart=True),
    "xstart_fixed_large": dict(predict_xstart=True, learn_sigma=False),
    "xstart_fixed_small": dict(predict_xstart=True, learn_sigma=False, sigma_small=True),
}
K_SHAPES = [(3, 3, 4, 6), (1, 4, 4, 8), (2, 16, 4, 32)]   # (B, F, C, H = W): 432, 1024 and 65 536 (XL/2) elements per sample


def kernel_grid():
    """-> [(spec, shape, index)]: {0, 1, T/2, T-1} of "50" on every shape, {0, 999} of "" on the first."""
    grid = [("50", sh, i) for sh in K_SHAPES for i in (0, 1, 25, 49)]
    return grid + [("", K_SHAPES[0], i) for i in (0, 999)]


def kernel_key(tag, clip, spec, shape, index):
    return f"K::{tag}::clip{int(clip)}::{spec or 'full'}::{shape[0]}x{shape[1]}x{shape[2]}x{shape[3] * shape[3]}::i{index}"


def kernel_x_start(shape):
    """x_start of a shape, with elements at exactly +-1.0 and at +-0.9995: both edge branches of the discretized likelihood
    (x < -0.999, x > 0.999) are taken by values the clamp alone would not produce."""
    B, F, C, H = shape
    g = torch.Generator("cpu").manual_seed(1000 + B * 100 + F)
    x0 = (torch.randn(B, F, C, H, H, generator=g) * 0.6).clamp(-1.0, 1.0)
    flat = x0.view(B, -1)
    for b in range(B):
        flat[b, 5], flat[b, 77], flat[b, 130], flat[b, 401] = 1.0, -1.0, 0.9995, -0.9995
    noise = torch.randn(B, F, C, H, H, generator=g)
    return x0, noise


def kernel_inputs(s, shape, index):
    """-> x_start, noise, x_t, model_out of one kernel-level case (``s``: a Schedule with the model types set)."""
    x0, noise = kernel_x_start(shape)
    B = shape[0]
    x_t = do.q_sample(s, x0, torch.full((B,), index, dtype=torch.int64), noise)
    oc = 2 * shape[2] if s.var_type == "learned_range" else shape[2]
    mo = do.synthetic_model(x_t, torch.full((B,), s.timestep_map[index], dtype=torch.int64), oc)
    return x0, noise, x_t, mo


def checksum(t):
    """The short fingerprint of a regenerated random input kept in the fixture: its sum and its first eight values."""
    f = t.detach().double().reshape(-1)
    return np.concatenate([[float(f.sum())], f[:8].numpy()])


def input_checksums():
    """{key: checksum} of every regenerated random input of the fixtures."""
    out = {}
    kw, cfg, sd, x0, y, noise = model_inputs()
    out["in::M::x0"], out["in::M::noise"] = checksum(x0), checksum(noise)
    out["in::M::weights"] = checksum(torch.cat([sd[k].reshape(-1)[:64] for k in sorted(sd)]))
    for sh in K_SHAPES:
        x0, nz = kernel_x_start(sh)
        out[f"in::K::{sh[0]}x{sh[1]}::x0"], out[f"in::K::{sh[0]}x{sh[1]}::noise"] = checksum(x0), checksum(nz)
    return out


# ---------------------------------------------------------------------------- the live reference (tools/make_bpd_golden.py, CPU test)
def reference_arrays():
    """Everything tests/golden/bpd.npz holds, computed by the reference objects (needs the reference checkout)."""
    from oracle import reference_loader as rl
    rd, rlatte = rl.load_reference_diffusion(), rl.load_reference_latte()
    arrays = dict(input_checksums())
    # M: the reference's own calc_bpd_loop on the reference's Latte
    kw, cfg, sd, x0, y, noise = model_inputs()
    model = rlatte.Latte(**kw)
    model.load_state_dict(sd)
    model.eval()
    d = rd.create_diffusion(M_SPEC)
    for clip in (True, False):
        state = torch.random.get_rng_state()
        torch.manual_seed(M_NOISE_SEED)
        with torch.no_grad():
            r = d.calc_bpd_loop(model, x0, clip_denoised=clip, model_kwargs=dict(y=y))
        torch.random.set_rng_state(state)
        for k in TABLES:
            arrays[f"M::clip{int(clip)}::{k}"] = r[k].numpy()
    # K: _vb_terms_bpd / _prior_bpd / _predict_eps_from_xstart on the synthetic model's outputs
    for tag, tkw in K_TYPES.items():
        for spec, shape, index in kernel_grid():
            d = rd.create_diffusion(spec, **tkw)
            s = do.Schedule(spec, **tkw)
            x_start, nz, _, _ = kernel_inputs(s, shape, index)
            t = torch.full((shape[0],), index, dtype=torch.int64)
            x_t = d.q_sample(x_start, t, noise=nz)
            oc = 2 * shape[2] if tkw.get("learn_sigma", True) else shape[2]
            fn = lambda x, tt, **k: do.synthetic_model(x, tt, oc)
            for clip in (True, False):
                out = d._vb_terms_bpd(fn, x_start=x_start, x_t=x_t, t=t, clip_denoised=clip, model_kwargs={})
                eps = d._predict_eps_from_xstart(x_t, t, out["pred_xstart"])
                arrays[kernel_key(tag, clip, spec, shape, index)] = np.stack([
                    out["output"].numpy(), ((out["pred_xstart"] - x_start) ** 2).mean(dim=[1, 2, 3, 4]).numpy(),
                    ((eps - nz) ** 2).mean(dim=[1, 2, 3, 4]).numpy()])
            if tag == "eps_learned":
                arrays[f"K::prior::{spec or 'full'}::{shape[0]}x{shape[1]}"] = d._prior_bpd(x_start).numpy()
    return arrays


# ---------------------------------------------------------------------------- measured differences of the GPU tests
def rel_max(got, want):
    """Worst entry-wise relative difference."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float((np.abs(got - want) / np.maximum(np.abs(want), 1e-30)).max())


def record(key, val):
    """The worst differences the GPU tests measured, per table and case, into the JSON file the environment variable
    LATTE_BPD_PARITY_JSON names (-> profiles/bpd_parity.json); without it the figures are only printed by the tests."""
    path = os.environ.get("LATTE_BPD_PARITY_JSON")
    if not path:
        return
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    tab = {}
    if os.path.exists(path):
        with open(path) as f:
            tab = json.load(f)
    tab[key] = val
    with open(path, "w") as f:
        json.dump(tab, f, indent=1, sort_keys=True)
