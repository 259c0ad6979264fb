"""fp32 restatement of DDIM inversion: ``GaussianDiffusion.ddim_reverse_sample`` (gaussian_diffusion.py:566-602) and the obvious
``for i in range(T)`` loop around it (the reference has none), plus the builders of the fixtures tests/golden/invert.npz is computed
on (tools/make_invert_golden.py).

Composed from the pinned CPU oracle (``oracle.diffusion_oracle``: ``p_mean_variance``, ``_coef``, ``Schedule``; ``oracle.latte_oracle``
as the denoiser); the model-level fixture M, the kernel-level types / shapes / inputs and the error helpers are those of
tests/bpd_reference.py.  tests/test_invert_reference.py pins the restatement to the committed fixture -- what the reference's own
``ddim_reverse_sample`` computed -- and, where the reference is present, to the live reference.

Fixture M: the 50-step chain on the two-block class-conditional Latte of bpd_reference (B = 2), clip_denoised on and off, and the same
model through ``forward_with_cfg`` at cfg_scale 4.0 on the doubled batch with null labels; kept: the sample after steps 0, 1, 24, 48,
49 and the last pred_xstart.  Fixtures K: single reverse steps on ``synthetic_model`` outputs for every ModelMeanType x ModelVarType,
clip on and off; kept per case: K_KEEP evenly spaced elements of sample / pred_xstart and the fp64 sum and sum of squares of each
(the XL/2-sized case alone would be 1 MB as tensors)."""
import contextlib
import json
import os

import numpy as np
import torch

import bpd_reference as br
from bpd_reference import K_SHAPES, K_TYPES, checksum, kernel_inputs, kernel_key, kernel_x_start, model_inputs, rel_max  # noqa: F401 (re-exported)
from oracle import diffusion_oracle as do
from oracle import latte_oracle as lo

M_SPEC = br.M_SPEC
M_CHECKPOINTS = (0, 1, 24, 48, 49)     # executed steps whose sample the fixture keeps
M_CFG_SCALE = 4.0
M_CASES = ("clip1", "clip0", "guided")  # guided: clip_denoised on, forward_with_cfg


@contextlib.contextmanager
def one_thread():
    """The fixture's bits are those of ONE CPU thread: torch splits an elementwise pass over more than 32 768 elements among its
    threads, and which elements then take the vector or the scalar form of sin / exp / erf depends on the split (as does MKL's GEMM
    blocking).  Both the generator and the tests compute under this."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(n)


# ---------------------------------------------------------------------------- the restatement
def alphas_cumprod_next(s):
    return np.append(s.alphas_cumprod[1:], 0.0)                                   # gd:174


def ddim_reverse_sample(s, model_out, x, i, clip_denoised=False, denoised_fn=None, cond_grad=None):
    """gd:566-602 for respaced index ``i``.  ``cond_grad`` = cond_fn(x, t) of condition_score (gd:589-590, :358-375)."""
    out = do.p_mean_variance(s, model_out, x, i, clip_denoised, denoised_fn)
    x0 = out["pred_xstart"]
    if cond_grad is not None:
        e = (do._coef(s.sqrt_recip_alphas_cumprod, i) * x - x0) / do._coef(s.sqrt_recipm1_alphas_cumprod, i)
        e = e - (1 - do._coef(s.alphas_cumprod, i)).sqrt() * cond_grad
        x0 = do._coef(s.sqrt_recip_alphas_cumprod, i) * x - do._coef(s.sqrt_recipm1_alphas_cumprod, i) * e
    eps = (do._coef(s.sqrt_recip_alphas_cumprod, i) * x - x0) / do._coef(s.sqrt_recipm1_alphas_cumprod, i)   # gd:593-596
    abn = do._coef(alphas_cumprod_next(s), i)
    return {"sample": x0 * torch.sqrt(abn) + torch.sqrt(1 - abn) * eps, "pred_xstart": x0}                 # gd:600


def invert_loop(s, model_fn, x, clip_denoised=True, start=0, end=None, denoised_fn=None, cond_fn=None):
    """``for i in range(start, end + 1)`` around the step.  ``model_fn(x, t_original int64[N])``.  -> [{"sample", "pred_xstart"}]."""
    end = s.num_timesteps - 1 if end is None else end
    trail = []
    for i in range(start, end + 1):
        t = torch.full((x.shape[0],), s.timestep_map[i], dtype=torch.int64)
        grad = None if cond_fn is None else cond_fn(x, t)
        r = ddim_reverse_sample(s, model_fn(x, t), x, i, clip_denoised, denoised_fn, grad)
        trail.append(r)
        x = r["sample"]
    return trail


def q_level(s, x0, noise, level):
    """q_sample at LEVEL ``level`` in 0 ... T: level i < T is respaced index i, level T is the noise itself (abar = 0)."""
    if level == s.num_timesteps:
        return noise.clone()
    return do.q_sample(s, x0, torch.full((x0.shape[0],), level, dtype=torch.int64), noise)


def consistent_model_out(s, x, i, x0, learned):
    """The output of the model that is consistent with (x0*, e*) at respaced index ``i``: eps = (x - sqrt(ab_i) x0*) / sqrt(1 - ab_i),
    or x0* itself for the x_start types; zero variance channels for the learned-range types."""
    if s.predict_xstart:
        out = x0.clone()
    else:
        out = (x - do._coef(s.sqrt_alphas_cumprod, i) * x0) / do._coef(s.sqrt_one_minus_alphas_cumprod, i)
    return torch.cat([out, torch.zeros_like(out)], dim=2) if learned else out


# ---------------------------------------------------------------------------- fixture M
def model_case(case):
    """-> (clip_denoised, guided) of an M case."""
    return case != "clip0", case == "guided"


def model_chain_inputs(case, extras=2, learn_sigma=True):
    """-> kw, cfg, sd, x [B or 2B, F, C, H, W], y | None, model_kwargs of the engine call."""
    kw, cfg, sd, x0, y, _ = model_inputs(extras, learn_sigma)
    _, guided = model_case(case)
    if guided:                                                                    # sample.py:88-94: doubled batch, null labels
        x0 = torch.cat([x0, x0], dim=0)
        y = torch.cat([y, torch.full_like(y, cfg.num_classes)], dim=0)
    return kw, cfg, sd, x0, y, guided


def model_restatement(case="clip1", extras=2, learn_sigma=True, spec=M_SPEC):
    """The restatement on fixture M (or its unconditional / fixed-variance variant) with the fp32 oracle as the denoiser
    -> {"sample": [5, B, ...] at M_CHECKPOINTS, "pred_xstart": [B, ...] of the last step} as numpy arrays."""
    kw, cfg, sd, x, y, guided = model_chain_inputs(case, extras, learn_sigma)
    s = do.Schedule(spec, learn_sigma=learn_sigma)
    if guided:
        fn = lambda xx, t: lo.latte_forward_with_cfg(sd, cfg, xx, t, y, M_CFG_SCALE)
    else:
        fn = lambda xx, t: lo.latte_forward(sd, cfg, xx, t, y)
    with torch.no_grad(), one_thread():
        trail = invert_loop(s, fn, x, model_case(case)[0])
    return {"sample": torch.stack([trail[k]["sample"] for k in M_CHECKPOINTS]).numpy(), "pred_xstart": trail[-1]["pred_xstart"].numpy()}


# ---------------------------------------------------------------------------- fixtures K
K_KEEP = 96


def kernel_grid():
    """-> [(spec, shape, index)]: {0, 1, 25, 48, 49} of "50" on every shape, {0, 999} of "" on the first.  Index T-1 is the
    alphas_cumprod_next = 0 row, index 0 the division by sqrt_recipm1 ~ 0.01."""
    grid = [("50", sh, i) for sh in K_SHAPES for i in (0, 1, 25, 48, 49)]
    return grid + [("", K_SHAPES[0], i) for i in (0, 999)]


def kernel_digest(r):
    """What the fixture keeps of a step's result -> (values float32 [2, K_KEEP], sums float64 [2, 2]), rows sample / pred_xstart."""
    vals, sums = [], []
    for k in ("sample", "pred_xstart"):
        f = r[k].detach().reshape(-1)
        idx = torch.from_numpy(np.linspace(0, f.numel() - 1, K_KEEP).astype(np.int64))
        vals.append(f[idx].float().cpu().numpy())
        d = f.double().cpu()
        sums.append([float(d.sum()), float((d * d).sum())])
    return np.stack(vals), np.array(sums)


def kernel_restatement(tag, clip, spec, shape, index):
    s = do.Schedule(spec, **K_TYPES[tag])
    with one_thread():
        _, _, x_t, mo = kernel_inputs(s, shape, index)
        return ddim_reverse_sample(s, mo, x_t, index, clip)


def input_checksums():
    """{key: checksum} of every regenerated random input of the fixtures (those of bpd_reference: the same generators)."""
    return {"in::" + k[4:]: v for k, v in br.input_checksums().items() if not k.endswith("M::noise")}


# ---------------------------------------------------------------------------- the live reference (tools/make_invert_golden.py, CPU test)
def reference_model_chain(case):
    """The reference's own ddim_reverse_sample stepped over create_diffusion("50") on the reference's Latte -> as model_restatement."""
    from oracle import reference_loader as rl
    rd, rlatte = rl.load_reference_diffusion(), rl.load_reference_latte()
    kw, cfg, sd, x, y, guided = model_chain_inputs(case)
    model = rlatte.Latte(**kw)
    model.load_state_dict(sd)
    model.eval()
    d = rd.create_diffusion(M_SPEC)
    fn, mk = (model.forward_with_cfg, dict(y=y, cfg_scale=M_CFG_SCALE)) if guided else (model.forward, dict(y=y))
    trail = []
    with torch.no_grad(), one_thread():
        for i in range(d.num_timesteps):
            r = d.ddim_reverse_sample(fn, x, torch.tensor([i] * x.shape[0]), clip_denoised=model_case(case)[0], model_kwargs=mk)
            trail.append(r)
            x = r["sample"]
    return {"sample": torch.stack([trail[k]["sample"] for k in M_CHECKPOINTS]).numpy(), "pred_xstart": trail[-1]["pred_xstart"].numpy()}


def reference_arrays():
    """Everything tests/golden/invert.npz holds, computed by the reference objects (needs the reference checkout)."""
    from oracle import reference_loader as rl
    rd = rl.load_reference_diffusion()
    arrays = dict(input_checksums())
    for case in M_CASES:
        r = reference_model_chain(case)
        arrays[f"M::{case}::sample"], arrays[f"M::{case}::pred_xstart"] = r["sample"], r["pred_xstart"]
    for tag, tkw in K_TYPES.items():
        for spec, shape, index in kernel_grid():
            d = rd.create_diffusion(spec, **tkw)
            s = do.Schedule(spec, **tkw)
            with one_thread():
                _, _, x_t, _ = kernel_inputs(s, shape, index)
            oc = 2 * shape[2] if tkw.get("learn_sigma", True) else shape[2]
            fn = lambda x, tt, **k: do.synthetic_model(x, tt, oc)
            t = torch.full((shape[0],), index, dtype=torch.int64)
            for clip in (True, False):
                with one_thread():
                    r = d.ddim_reverse_sample(fn, x_t, t, clip_denoised=clip, model_kwargs={})
                key = kernel_key(tag, clip, spec, shape, index)
                arrays[key], arrays[key + "::sums"] = kernel_digest(r)
    return arrays


# ---------------------------------------------------------------------------- measured differences of the GPU tests
def record(key, val):
    """The worst differences the GPU tests measured into the JSON file the environment variable LATTE_INVERT_PARITY_JSON names
    (-> profiles/invert_parity.json); without it the figures are only printed by the tests."""
    path = os.environ.get("LATTE_INVERT_PARITY_JSON")
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
