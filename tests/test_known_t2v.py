"""Known-region sampling on the text-to-video chain: ``LattePipeline.__call__(known_latents=, known_mask=)`` on the tiny_t2v fixture and
the pipe of tests/test_t2v_schedulers.py, the first frame known.  The fused call (``latte_t2v_guided_ddim_loop_known``) against the
Python loop with ``latte_known_blend`` at the 1e-5 that file holds its fused chains to; against the fp32 oracle denoiser loop with the
blend written in torch at the project's 1e-3; the known part of the result exact; the other schedulers refused."""
import pytest
import torch

import latte_amd
from latte_amd.schedulers import DDIMScheduler, DPMSolverMultistepScheduler, EulerDiscreteScheduler
from _util import rel_l2
from test_t2v_schedulers import _fixture, _model

pytestmark = pytest.mark.gpu
STEPS, SCALE = 5, 4.5
INVALID = 1


@pytest.fixture(scope="module")
def t2v_pipe():
    cfg, sd = _fixture()
    pipe = latte_amd.LattePipeline(transformer=_model(cfg, sd, max_batch=4), scheduler=DDIMScheduler()).to("cuda")
    return cfg, sd, pipe


def _inputs(cfg, b):
    g = torch.Generator("cpu").manual_seed(9)
    pe, ne = torch.randn(b, 6, cfg.caption_channels, generator=g), torch.randn(b, 6, cfg.caption_channels, generator=g)
    shape = (b, 4, cfg.video_length, cfg.sample_size, cfg.sample_size)
    lat = torch.randn(shape, generator=g)
    known = (torch.randn(shape, generator=g) * 0.6).clamp(-1, 1)
    mask = latte_amd.known_mask((b, cfg.video_length, cfg.sample_size, cfg.sample_size), frames=[0])
    return pe, ne, lat, known, mask


def _run(pipe, pe, ne, lat, known, mask, fused, seed=21, **kw):
    pipe.allow_fused_loop = fused
    try:
        return pipe(prompt_embeds=pe, negative_prompt_embeds=ne, num_inference_steps=STEPS, guidance_scale=SCALE, latents=lat,
                    generator=torch.Generator("cpu").manual_seed(seed), output_type="latents", known_latents=known, known_mask=mask, **kw).video
    finally:
        pipe.allow_fused_loop = True


def test_fused_call_matches_the_python_loop_and_keeps_the_known_part(t2v_pipe):
    cfg, sd, pipe = t2v_pipe
    pipe.scheduler = DDIMScheduler()
    pe, ne, lat, known, mask = _inputs(cfg, 2)
    tr = pipe.transformer
    calls = {"fused": 0, "blend": 0}
    lib = latte_amd.load_library()
    real_blend = lib.latte_known_blend

    def spy(*a, **kw):
        calls["fused"] += 1
        return type(tr).guided_ddim_loop_known(tr, *a, **kw)

    def blend_spy(*a):
        calls["blend"] += 1
        return real_blend(*a)

    tr.guided_ddim_loop_known = spy
    lib.latte_known_blend = blend_spy
    try:
        fused = _run(pipe, pe, ne, lat, known, mask, True)
        assert calls == {"fused": 1, "blend": 0}, calls                      # ONE engine call
        stepped = _run(pipe, pe, ne, lat, known, mask, False)
        assert calls == {"fused": 1, "blend": STEPS + 1}, calls              # one launch before the first step and after every step
    finally:
        del tr.guided_ddim_loop_known
        lib.latte_known_blend = real_blend
    err = rel_l2(fused, stepped)
    print(f"known-region DDIM chain, fused vs Python loop rel-L2 {err:.3e}")
    assert torch.isfinite(fused).all() and err < 1e-5
    m5 = mask[:, None].expand_as(fused).cuda()
    for out in (fused, stepped):
        assert torch.equal(out[m5 == 1], known.cuda()[m5 == 1]) and not torch.equal(out[m5 == 0], known.cuda()[m5 == 0])
    plain = pipe(prompt_embeds=pe, negative_prompt_embeds=ne, num_inference_steps=STEPS, guidance_scale=SCALE, latents=lat, output_type="latents").video
    assert not torch.equal(plain, fused)
    # an all-zero mask is the plain chain bit for bit (the generator's draws are not used by it)
    zero = _run(pipe, pe, ne, lat, known, torch.zeros_like(mask), True)
    assert torch.equal(zero, plain)


def test_chain_matches_the_oracle_denoiser_loop(t2v_pipe):
    from oracle import latte_t2v_oracle as to
    cfg, sd, pipe = t2v_pipe
    pipe.scheduler = DDIMScheduler()
    pe, ne, lat, known, mask = _inputs(cfg, 1)
    got = _run(pipe, pe, ne, lat, known, mask, True)
    sch = DDIMScheduler()
    sch.set_timesteps(STEPS)
    gen = torch.Generator("cpu").manual_seed(21)
    noise = [torch.randn(lat.shape, generator=gen) for _ in range(STEPS)]          # the pipeline's draws, in slab order
    ratio = sch.num_train_timesteps // STEPS
    m5 = mask[:, None]

    def blend(x, abar, z):
        kn = known if z is None else abar ** 0.5 * known + (1.0 - abar) ** 0.5 * z
        return torch.where(m5 == 1, kn, x)

    want = blend(lat.clone(), float(sch.alphas_cumprod[int(sch.timesteps[0])]), noise[0])
    with torch.no_grad():
        for k, t in enumerate(sch.timesteps):
            out = to.latte_t2v_forward(sd, cfg, torch.cat([want] * 2), t.reshape(1).expand(2), torch.cat([ne, pe]))
            unc, txt = out.chunk(2)
            eps = (unc + SCALE * (txt - unc)).chunk(2, dim=1)[0]
            want = sch.step(eps, t, want, return_dict=False)[0]
            prev = int(t) - ratio
            a_prev = float(sch.alphas_cumprod[prev]) if prev >= 0 else float(sch.final_alpha_cumprod)
            want = blend(want, a_prev, noise[k + 1] if k + 1 < STEPS else None)
    err = rel_l2(got, want)
    print(f"known-region DDIM chain vs oracle loop rel-L2 {err:.3e}")
    assert err < 1e-3
    assert torch.equal(got.cpu()[m5.expand_as(got) == 1], known[m5.expand_as(got) == 1])


def test_other_schedulers_and_bad_arguments_are_refused(t2v_pipe):
    from latte_amd._lib import ptr, stream_ptr
    cfg, sd, pipe = t2v_pipe
    pe, ne, lat, known, mask = _inputs(cfg, 1)
    for cls in (EulerDiscreteScheduler, DPMSolverMultistepScheduler):
        pipe.scheduler = cls()
        with pytest.raises(latte_amd.LatteError, match="DDIMScheduler"):
            _run(pipe, pe, ne, lat, known, mask, True)
    pipe.scheduler = DDIMScheduler()
    with pytest.raises(latte_amd.LatteError, match="DDIMScheduler"):
        _run(pipe, pe, ne, lat, known, mask, True, eta=0.5)
    with pytest.raises(latte_amd.LatteError, match="come together"):
        _run(pipe, pe, ne, lat, known, None, True)
    with pytest.raises(latte_amd.LatteError, match="known_mask"):
        _run(pipe, pe, ne, lat, known, mask[:, :2], True)
    # the engine entry point: every refusal before the first launch, the latents untouched
    import numpy as np
    _run(pipe, pe, ne, lat, known, mask, True)                               # installs the text context of the pair
    m, lib = pipe.transformer, latte_amd.load_library()
    x = lat.cuda().contiguous()
    before = x.clone()
    kn, mk = known.cuda().contiguous(), mask.cuda().contiguous()
    nz = torch.randn((2,) + tuple(lat.shape), device="cuda")
    ts = np.array([500, 0], dtype=np.int64)
    at, ap = np.array([0.3, 0.9]), np.array([0.9, 1.0])
    bad_at = np.array([0.3, 1.5])
    for args, text in (((ptr(None), ptr(mk), ptr(nz)), b"required"), ((ptr(kn), ptr(None), ptr(nz)), b"required"),
                       ((ptr(kn), ptr(mk), ptr(None)), b"required")):
        rc = lib.latte_t2v_guided_ddim_loop_known(m._h, ptr(x), 1, 2, ts.ctypes.data, at.ctypes.data, ap.ctypes.data, SCALE, *args, 1, stream_ptr())
        assert rc == INVALID and text in lib.latte_last_error()
    rc = lib.latte_t2v_guided_ddim_loop_known(m._h, ptr(x), 1, 2, ts.ctypes.data, bad_at.ctypes.data, ap.ctypes.data, SCALE, ptr(kn), ptr(mk),
                                              ptr(nz), 1, stream_ptr())
    assert rc == INVALID and b"alpha out of range" in lib.latte_last_error()
    torch.cuda.synchronize()
    assert torch.equal(x, before)
