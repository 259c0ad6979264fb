"""Training losses, forward evaluation (first slice): q_sample and
GaussianDiffusion.training_losses (gaussian_diffusion.py:216-229,686-795) for every loss / model type create_diffusion
builds.  The fixture tests/golden/training_losses.npz holds the REFERENCE's outputs (oracle/make_golden.py:training); on CPU
the oracle restatement must reproduce it bit for bit, on the GPU the engine must match it."""
import os

import numpy as np
import pytest
import torch

from _util import GOLDEN, pinned, rel_l2
from oracle import diffusion_oracle as do
from oracle.make_golden import TRAINING_CASES, training_inputs

LOSS_OF = {"mse_learned": "mse", "rescaled_mse_learned_100": "rescaled_mse", "rescaled_kl_learned": "rescaled_kl",
           "mse_fixed_large": "mse", "mse_xstart_learned": "mse"}


def _golden():
    return np.load(os.path.join(GOLDEN, "training_losses.npz"))


def _oracle_training_losses(case):
    """-> (q_sample, training_losses terms) of the oracle on the fixture's inputs; run through pinned()."""
    tag, kw, spec = case
    s = do.Schedule(spec, predict_xstart=kw.get("predict_xstart", False), learn_sigma=kw.get("learn_sigma", True))
    x0, noise, t = training_inputs(s.num_timesteps)
    oc = 8 if kw.get("learn_sigma", True) else 4
    terms = do.training_losses(s, lambda x, tt: do.synthetic_model(x, tt, oc), x0, t, noise, LOSS_OF[tag])
    return do.q_sample(s, x0, t, noise).numpy(), {k: v.numpy() for k, v in terms.items()}


@pytest.mark.parametrize("case", TRAINING_CASES, ids=lambda c: c[0])
def test_oracle_training_losses_bit_identical_to_reference(case):
    """The terms on the pinned arithmetic (tests/_util.pinned) against the reference's on it (oracle/make_golden.py:pinned_reference)."""
    tag, kw, spec = case
    z = _golden()
    p = np.load(os.path.join(GOLDEN, "pinned_reference.npz"))
    x_t, terms = pinned(_oracle_training_losses, case)
    assert torch.equal(torch.from_numpy(x_t), torch.from_numpy(z[f"{tag}::x_t"]))
    keys = {k.split("::")[1] for k in z.files if k.startswith(tag + "::")} - {"x_t"}
    assert set(terms) == keys and {k for k in p.files if k.startswith(f"training::{tag}::")} == {f"training::{tag}::{k}" for k in keys}
    for k in keys:
        assert torch.equal(torch.from_numpy(terms[k]), torch.from_numpy(p[f"training::{tag}::{k}"])), (tag, k)
    x0, _, t = training_inputs(do.Schedule(spec).num_timesteps)
    assert int(t[0]) == 0 and float(x0.abs().max()) == 1.0        # the fixture exercises the decoder-NLL and tail branches


def test_shim_maps_create_diffusion_arguments_to_loss_types(lib):
    import latte_amd
    assert latte_amd.create_diffusion("").loss_type == "mse"
    assert latte_amd.create_diffusion("", rescale_learned_sigmas=True).loss_type == "rescaled_mse"
    assert latte_amd.create_diffusion("", use_kl=True).loss_type == "rescaled_kl"
    d = latte_amd.create_diffusion("10")
    assert np.allclose(d.sqrt_alphas_cumprod ** 2 + d.sqrt_one_minus_alphas_cumprod ** 2, 1.0, atol=1e-15)
    if not torch.cuda.is_available():
        with pytest.raises(latte_amd.LatteError):
            d.training_losses(lambda x, t: x, torch.zeros(1, 4, 4, 8, 8), torch.zeros(1, dtype=torch.int64))


@pytest.mark.gpu
@pytest.mark.parametrize("case", TRAINING_CASES, ids=lambda c: c[0])
def test_engine_training_losses_match_reference(case):
    """Tolerance: the per-element arithmetic is the reference's fp32 op sequence, but expf / logf / tanhf are the device's
    implementations and the mean is a different summation order: 2e-5 relative on every term (measured ~1e-6)."""
    import latte_amd
    tag, kw, spec = case
    z = _golden()
    d = latte_amd.create_diffusion(spec, **kw)
    x0, noise, t = training_inputs(d.num_timesteps)
    oc = 8 if kw.get("learn_sigma", True) else 4
    x0d, nzd, td = x0.cuda(), noise.cuda(), t.cuda()
    xt = d.q_sample(x0d, td, nzd)
    assert rel_l2(xt, torch.from_numpy(z[f"{tag}::x_t"])) < 1e-7
    seen = []

    def model(x, tt, **k):
        seen.append(tt.cpu())
        return do.synthetic_model(x, tt, oc)

    terms = d.training_losses(model, x0d, td, model_kwargs={}, noise=nzd)
    assert torch.equal(seen[0], torch.tensor(d.timestep_map)[t])          # the model sees ORIGINAL timesteps (rs:125-130)
    keys = {k.split("::")[1] for k in z.files if k.startswith(tag + "::")} - {"x_t"}
    assert set(terms) == keys
    for k in keys:
        want = torch.from_numpy(z[f"{tag}::{k}"])
        got = terms[k].cpu()
        assert torch.isfinite(got).all()
        assert float(((got - want).abs() / want.abs().clamp_min(1e-12)).max()) < 2e-5, (tag, k, got, want)


@pytest.mark.gpu
def test_training_losses_on_the_engine_denoiser():
    """train.py:224-226 with the engine model as the callable: per-sample timesteps, class labels, learned sigma."""
    import latte_amd
    from _util import engine_model, load_golden_model
    from oracle import latte_oracle as lo
    from _util import oracle_config
    kw, sd, r = load_golden_model("tiny_classcond")
    m = engine_model(kw, sd, "f16")
    d = latte_amd.create_diffusion("")
    g = torch.Generator("cpu").manual_seed(12)
    x0 = torch.randn(2, kw["num_frames"], 4, kw["input_size"], kw["input_size"], generator=g).clamp(-1, 1)
    nz = torch.randn(x0.shape, generator=g)
    t = torch.tensor([0, 731])
    y = torch.tensor([3, 1])
    got = d.training_losses(m, x0.cuda(), t.cuda(), model_kwargs=dict(y=y.cuda()), noise=nz.cuda())
    s = do.Schedule("")
    cfg = oracle_config(kw)
    want = do.training_losses(s, lambda x, tt: lo.latte_forward(sd, cfg, x, tt, y), x0, t, nz, "mse")
    for k in ("mse", "vb", "loss"):
        assert float(((got[k].cpu() - want[k]).abs() / want[k].abs()).max()) < 1e-3, k
