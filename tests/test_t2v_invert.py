"""DDIM inversion for text-to-video: ``DDIMInverseScheduler`` (the algebraic inverse of this project's DDIM chain, as an
``engine_plan()`` table) on the CPU in fp64, and ``LattePipeline.invert`` on tests/golden/tiny_t2v.npz, built exactly as
tests/test_t2v_schedulers.py builds its pipeline: the fused chain against the step-by-step loop, both against the oracle denoiser
(``oracle.latte_t2v_oracle``) stepped with the same scheduler, and the unguided path.

The scheduler is memory-derived and not pinned against diffusers; what is pinned is that it inverts the DDIM update exactly for a
constant eps, which is the property inversion rests on."""
import json
import os

import numpy as np
import pytest
import torch

import latte_amd
from latte_amd.schedulers import DDIMInverseScheduler, DDIMScheduler, P_C0, P_CX, P_IN, P_MEPS, P_MX, P_T
from _util import GOLDEN, rel_l2


def _ddim_down(sch_inv, n, x, eps):
    """The DDIM chain (eq. 12 at eta = 0) over the inverse scheduler's own timestep set, descending, for a fixed eps: what
    ``DDIMScheduler.step`` computes on the "leading" set, written out so that the "trailing" set is covered too."""
    sch_inv.set_timesteps(n)
    ts = [int(t) for t in sch_inv.timesteps][::-1]
    ab = sch_inv.alphas_cumprod
    for k, t in enumerate(ts):
        a_t = float(ab[t])
        a_prev = float(ab[ts[k + 1]]) if k + 1 < len(ts) else sch_inv.final_alpha_cumprod
        x0 = (x - (1.0 - a_t) ** 0.5 * eps) / a_t ** 0.5
        x = a_prev ** 0.5 * x0 + (1.0 - a_prev) ** 0.5 * eps
    return x


def _up(sch, n, x, model):
    sch.set_timesteps(n)
    for t in sch.timesteps:
        x = sch.step(model(sch.scale_model_input(x, t), t), t, x, return_dict=False)[0]
    return x


@pytest.mark.parametrize("n", [1, 7, 50])
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("spacing", ["leading", "trailing"])
@pytest.mark.parametrize("alpha_to_one", [True, False])
def test_inverts_the_ddim_chain_for_a_constant_eps(spacing, offset, n, alpha_to_one):
    g = torch.Generator("cpu").manual_seed(n)
    x_start = torch.randn(2, 4, 3, 5, 5, generator=g, dtype=torch.float64)
    eps = torch.randn(2, 4, 3, 5, 5, generator=g, dtype=torch.float64)
    inv = DDIMInverseScheduler(timestep_spacing=spacing, steps_offset=offset, set_alpha_to_one=alpha_to_one)
    if spacing == "leading":     # this project's DDIMScheduler itself (its spacing is the leading one)
        ddim = DDIMScheduler(steps_offset=offset, set_alpha_to_one=alpha_to_one)
        ddim.set_timesteps(n)
        inv.set_timesteps(n)
        assert [int(t) for t in ddim.timesteps] == [int(t) for t in inv.timesteps][::-1]
        x = x_start
        for t in ddim.timesteps:
            x = ddim.step(eps, t, x, return_dict=False)[0]
        assert torch.allclose(x, _ddim_down(inv, n, x_start, eps), rtol=0, atol=1e-12 * float(x.abs().max()))
    else:
        x = _ddim_down(inv, n, x_start, eps)
    back = _up(inv, n, x, lambda xx, t: eps)
    assert float((back - x_start).abs().max()) <= 1e-12 * float(x_start.abs().max())
    assert float((x - x_start).abs().max()) > 1e-3 or n == 1 and not alpha_to_one and offset == 0     # the chain did move x


@pytest.mark.parametrize("spacing", ["leading", "trailing"])
def test_engine_plan_rows_reproduce_step(spacing):
    sch = DDIMInverseScheduler(timestep_spacing=spacing)
    sch.set_timesteps(7)
    plan = sch.engine_plan()
    assert plan.shape == (7, 12)
    assert np.all(plan[:, P_IN] == 1.0) and np.all(plan[:, P_MX] == 0.0) and np.all(plan[:, P_MEPS] == 1.0) and np.all(plan[:, 6:] == 0.0)
    assert [int(t) for t in plan[:, P_T]] == [int(t) for t in sch.timesteps]
    g = torch.Generator("cpu").manual_seed(3)
    x = torch.randn(1, 4, 2, 3, 3, generator=g, dtype=torch.float64)
    want = x.clone()
    for j, t in enumerate(sch.timesteps):
        eps = torch.sin(want * 1.3 + 0.01 * float(t))
        x_plan = plan[j, P_CX] * want + plan[j, P_C0] * (plan[j, P_MX] * want + plan[j, P_MEPS] * eps)
        want = sch.step(eps, t, want, return_dict=False)[0]
        assert torch.equal(x_plan, want)
    # levels: row j leaves a_from = 1 (j = 0) or abar[u_{j-1}] and enters abar[u_j]
    ab = sch.alphas_cumprod
    a = [1.0] + [float(ab[int(t)]) for t in sch.timesteps]
    assert np.allclose(plan[:, P_CX], [(a[j + 1] / a[j]) ** 0.5 for j in range(7)], rtol=1e-15)


def test_timesteps_ascend_and_step_past_the_end_raises():
    sch = DDIMInverseScheduler()
    with pytest.raises(ValueError, match="set_timesteps"):
        sch.engine_plan()
    for n in (1, 7, 50):
        sch.set_timesteps(n)
        ts = [int(t) for t in sch.timesteps]
        assert len(ts) == n and ts == sorted(set(ts)) and ts[0] >= 0 and ts[-1] < 1000
    fwd = DDIMScheduler()
    fwd.set_timesteps(50)
    assert ts == [int(t) for t in fwd.timesteps][::-1]
    assert sch.init_noise_sigma == 1.0 and sch.order == 1
    x = torch.zeros(1, 4, 1, 2, 2)
    for t in sch.timesteps:
        x = sch.step(x, t, x, return_dict=False)[0]
    with pytest.raises(IndexError):
        sch.step(x, sch.timesteps[-1], x)
    with pytest.raises(ValueError, match="clip_sample"):
        DDIMInverseScheduler(clip_sample=True)


# ------------------------------------------------------------------------------------------------ the pipeline on the GPU
def _fixture():
    from oracle import latte_t2v_oracle as to
    z = np.load(os.path.join(GOLDEN, "tiny_t2v.npz"))
    cfg = to.T2VConfig(**json.loads(bytes(z["cfg_json"]).decode()))
    sd = {k[4:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd::")}
    return cfg, sd


@pytest.fixture(scope="module")
def t2v_pipe():
    cfg, sd = _fixture()
    m = latte_amd.LatteT2V(num_attention_heads=cfg.num_attention_heads, attention_head_dim=cfg.attention_head_dim,
                           in_channels=cfg.in_channels, out_channels=cfg.out_channels, num_layers=cfg.num_layers,
                           sample_size=cfg.sample_size, patch_size=cfg.patch_size, cross_attention_dim=cfg.cross_attention_dim,
                           caption_channels=cfg.caption_channels, video_length=cfg.video_length, compute_dtype="f16", max_batch=4)
    m.load_state_dict(sd)
    return cfg, sd, latte_amd.LattePipeline(transformer=m, scheduler=DDIMScheduler()).to("cuda")


def _inputs(cfg, b):
    g = torch.Generator("cpu").manual_seed(9)
    pe, ne = torch.randn(b, 6, cfg.caption_channels, generator=g), torch.randn(b, 6, cfg.caption_channels, generator=g)
    lat = torch.randn(b, 4, cfg.video_length, cfg.sample_size, cfg.sample_size, generator=g) * 0.5
    return pe, ne, lat


def _oracle_invert(cfg, sd, lat, pe, ne, steps, scale):
    from oracle import latte_t2v_oracle as to
    sch = DDIMInverseScheduler()
    sch.set_timesteps(steps)
    x = lat.clone()
    b = lat.shape[0]
    with torch.no_grad():
        for t in sch.timesteps:
            if scale > 1.0:
                out = to.latte_t2v_forward(sd, cfg, torch.cat([x] * 2), t.reshape(1).expand(2 * b), torch.cat([ne, pe]))
                unc, txt = out.chunk(2)
                out = unc + scale * (txt - unc)
            else:
                out = to.latte_t2v_forward(sd, cfg, x, t.reshape(1).expand(b), pe)
            x = sch.step(out.chunk(2, dim=1)[0] if cfg.out_channels == 2 * cfg.in_channels else out, t, x, return_dict=False)[0]
    return x


@pytest.mark.gpu
def test_invert_fused_chain_matches_step_by_step_and_is_one_call(t2v_pipe):
    cfg, sd, pipe = t2v_pipe
    pe, ne, lat = _inputs(cfg, 2)
    out, calls = {}, {True: 0, False: 0}
    tr = pipe.transformer
    for fused in (True, False):
        pipe.allow_fused_loop = fused

        def spy(*a, _fused=fused, **kw):
            calls[_fused] += 1
            return type(tr).guided_linear_loop(tr, *a, **kw)

        tr.guided_linear_loop = spy
        try:
            out[fused] = pipe.invert(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, num_inference_steps=6, guidance_scale=4.5)
        finally:
            del tr.guided_linear_loop
    pipe.allow_fused_loop = True
    assert calls == {True: 1, False: 0}
    err = rel_l2(out[True], out[False])
    print(f"invert: fused chain vs step-by-step loop rel-L2 {err:.3e}")
    assert out[True].shape == lat.shape and torch.isfinite(out[True]).all() and err < 1e-5
    assert rel_l2(out[True], lat) > 1e-2 and type(pipe.scheduler) is DDIMScheduler          # moved; the pipeline's scheduler is untouched


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [4.5, 1.0], ids=["guided", "unguided"])
def test_invert_matches_the_oracle_denoiser_loop(t2v_pipe, scale):
    cfg, sd, pipe = t2v_pipe
    pe, ne, lat = _inputs(cfg, 1)
    tr, calls = pipe.transformer, [0]

    def spy(*a, **kw):
        calls[0] += 1
        return type(tr).guided_linear_loop(tr, *a, **kw)

    tr.guided_linear_loop = spy
    try:
        got = pipe.invert(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, num_inference_steps=4, guidance_scale=scale)
    finally:
        del tr.guided_linear_loop
    assert calls[0] == (1 if scale > 1.0 else 0)            # the unguided path steps LatteT2V.forward, without a guidance pair
    want = _oracle_invert(cfg, sd, lat, pe, ne, 4, scale)
    err = rel_l2(got, want)
    print(f"invert scale {scale}: engine vs oracle loop rel-L2 {err:.3e}")
    assert err < 1e-3


@pytest.mark.gpu
def test_invert_argument_errors(t2v_pipe):
    cfg, sd, pipe = t2v_pipe
    pe, ne, lat = _inputs(cfg, 1)
    with pytest.raises(ValueError, match="latents"):
        pipe.invert(prompt_embeds=pe)
    with pytest.raises(ValueError, match="prompt"):
        pipe.invert(latents=lat)
    with pytest.raises(ValueError, match="latents must be"):
        pipe.invert(prompt_embeds=pe, latents=lat[:, :3])
    with pytest.raises(ValueError, match="one prompt per clip"):
        pipe.invert(prompt_embeds=torch.cat([pe, pe]), latents=lat)
