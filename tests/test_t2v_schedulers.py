"""Euler, Euler-ancestral, Heun and DPM-Solver++ for the text-to-video chain: the four scheduler classes of latte_amd.schedulers
(memory-derived, unpinned against diffusers -- so they are pinned to the DDIM stand-in, to exact solutions and to their orders of
convergence), their engine_plan() tables, the guided step kernel behind latte_t2v_guided_linear_loop and the fused chain.

CPU tests: fp64, linear betas 1e-4 .. 0.02, around the analytic eps-model of Gaussian data N(mu, s^2),
eps*(x, t) = sqrt(1 - abar) (x - sqrt(abar) mu) / (abar s^2 + 1 - abar), whose probability-flow solution from the first timestep is
mu + s / sqrt(abar_0 s^2 + 1 - abar_0) (x_T - sqrt(abar_0) mu)."""
import json
import os

import numpy as np
import pytest
import torch

import latte_amd
from latte_amd.schedulers import (PLAN_COLS, DDIMScheduler, DPMSolverMultistepScheduler, EulerAncestralDiscreteScheduler,
                                  EulerDiscreteScheduler, HeunDiscreteScheduler)
from _util import GOLDEN, rel_l2

CLASSES = [EulerDiscreteScheduler, EulerAncestralDiscreteScheduler, HeunDiscreteScheduler, DPMSolverMultistepScheduler]
KDIFF = (EulerDiscreteScheduler, EulerAncestralDiscreteScheduler, HeunDiscreteScheduler)
MU, S = 0.7, 0.5
X_T = torch.tensor([1.3, -0.4, 0.2], dtype=torch.float64)


def _abar(sch, t):
    return float(sch.alphas_cumprod[int(t)])


def gaussian_eps(sch, x_scaled, t, mu=MU, s=S):
    """eps* at timestep t on the MODEL INPUT (x itself for DPM-Solver++ / DDIM, x~ / sqrt(sigma^2 + 1) = x for the k-diffusion family)."""
    a = _abar(sch, t)
    return (1.0 - a) ** 0.5 * (x_scaled - a ** 0.5 * mu) / (a * s * s + 1.0 - a)


def exact_answer(sch, x_t, mu=MU, s=S):
    a0 = _abar(sch, sch.timesteps[0])
    return mu + s / (a0 * s * s + 1.0 - a0) ** 0.5 * (x_t - a0 ** 0.5 * mu)


def run_steps(sch, n, x_t, model, generator=None, trace=None):
    """The scale_model_input / step loop of LattePipeline; x_t is the x-space start (x~_0 = x_T / sqrt(abar_0) = init_noise_sigma * unit
    noise for the k-diffusion family)."""
    sch.set_timesteps(n)
    x = x_t.clone()
    if isinstance(sch, KDIFF):
        x = x / _abar(sch, sch.timesteps[0]) ** 0.5
    kw = {"generator": generator} if generator is not None else {}
    for t in sch.timesteps:
        eps = model(sch, sch.scale_model_input(x, t), t)
        x = sch.step(eps, t, x, return_dict=False, **kw)[0]
        if trace is not None:
            trace.append(x.clone())
    return x


def run_plan(sch, n, x_t, model, noise=None):
    """The rows of engine_plan() applied in numpy: the step kernel's formula and the engine's ring of three remembered outputs, fp64."""
    sch.set_timesteps(n)
    plan = sch.engine_plan()
    x = x_t.numpy().copy()
    if isinstance(sch, KDIFF):
        x = x / _abar(sch, sch.timesteps[0]) ** 0.5
    hist = [None, None, None]
    for k, (t, in_scale, m_x, m_eps, c_x, c0, c1, c2, c3, c_noise, push, rsv) in enumerate(plan):
        assert t == int(t) and rsv == 0.0 and push in (0.0, 1.0)
        eps = model(sch, torch.from_numpy(in_scale * x), int(t)).numpy()
        m0 = m_x * x + m_eps * eps
        new = c_x * x + c0 * m0
        for cj, hj in zip((c1, c2, c3), hist):
            if cj != 0.0:
                new = new + cj * hj
        if c_noise != 0.0:
            new = new + c_noise * noise[k]
        x = new
        if push:
            hist = [m0] + hist[:2]
    return torch.from_numpy(x)


# ------------------------------------------------------------------------------------------------ 1. pins to the DDIM stand-in
@pytest.mark.parametrize("spacing", ["leading", "trailing"])
def test_first_order_dpm_and_euler_are_the_ddim_chain(spacing):
    n = 10
    ddim = DDIMScheduler()
    ddim.set_timesteps(n)                                    # its step only needs the stride T // n = 100, which both spacings have
    dpm = DPMSolverMultistepScheduler(solver_order=1, timestep_spacing=spacing)
    eul = EulerDiscreteScheduler(timestep_spacing=spacing)
    dpm.set_timesteps(n)
    want, x = [], X_T.clone()
    for t in dpm.timesteps:
        x = ddim.step(gaussian_eps(ddim, x, t), t, x, return_dict=False)[0]
        want.append(x.clone())
    got = []
    run_steps(dpm, n, X_T, gaussian_eps, trace=got)
    err = max(float((g - w).abs().max()) for g, w in zip(got, want))
    print(f"DPM-Solver++ order 1 vs DDIM chain [{spacing}]: {err:.2e}")
    assert err < 1e-12
    got = []
    last = run_steps(eul, n, X_T, gaussian_eps, trace=got)
    ab = [_abar(eul, t) for t in eul.timesteps[1:]] + [1.0]  # abar the chain stands at after each step
    err = max(float((g * a ** 0.5 - w).abs().max()) for g, a, w in zip(got, ab, want))
    print(f"Euler x sqrt(abar) vs DDIM chain [{spacing}]: {err:.2e}")
    assert err < 1e-12 and float((last - want[-1]).abs().max()) < 1e-12


# ------------------------------------------------------------------------------------------------ 2. exactness
@pytest.mark.parametrize("n,spacing", [(7, "leading"), (20, "trailing")])
def test_dpm2m_returns_the_mean_of_a_point_mass(n, spacing):
    sch = DPMSolverMultistepScheduler(timestep_spacing=spacing)
    got = run_steps(sch, n, X_T, lambda s, x, t: gaussian_eps(s, x, t, s=0.0))
    err = float((got - MU).abs().max())
    print(f"DPM++ 2M, s = 0, n = {n} {spacing}: {err:.2e}")
    assert err < 1e-12


@pytest.mark.parametrize("cls", [EulerDiscreteScheduler, HeunDiscreteScheduler])
def test_constant_eps_is_integrated_exactly(cls):
    sch = cls()
    sch.set_timesteps(9)
    sigma0 = ((1.0 - _abar(sch, sch.timesteps[0])) / _abar(sch, sch.timesteps[0])) ** 0.5
    x0 = X_T / _abar(sch, sch.timesteps[0]) ** 0.5
    got = run_steps(sch, 9, X_T, lambda s, x, t: torch.full_like(x, 0.3))
    err = float((got - (x0 - sigma0 * 0.3)).abs().max())
    print(f"{cls.__name__}, constant eps: {err:.2e}")
    assert err < 1e-12


# ------------------------------------------------------------------------------------------------ 3. order of convergence
@pytest.mark.parametrize("cls,ratio", [(EulerDiscreteScheduler, 3.0), (HeunDiscreteScheduler, 10.0), (DPMSolverMultistepScheduler, 8.0)])
def test_order_of_convergence(cls, ratio):
    err = {}
    for n in (20, 80):
        sch = cls()
        got = run_steps(sch, n, X_T, gaussian_eps)
        err[n] = float((got - exact_answer(sch, X_T)).abs().max())
        if cls is HeunDiscreteScheduler:
            assert len(sch.timesteps) == 2 * n - 1          # 39 / 159 evaluations
    print(f"{cls.__name__}: e20 = {err[20]:.3e}, e80 = {err[80]:.3e}, ratio {err[20] / err[80]:.2f}")
    assert err[20] / err[80] > ratio
    assert err[80] < 0.03


# ------------------------------------------------------------------------------------------------ 4. Euler-ancestral
def test_euler_ancestral_variances():
    sch = EulerAncestralDiscreteScheduler()
    final = []
    for n in (250, 1000):
        sch.set_timesteps(n)
        plan = sch.engine_plan()
        sig = np.append(1.0 / plan[:, 1] ** 2 - 1.0, 0.0) ** 0.5                   # sigma_i back from in_scale = 1 / sqrt(sigma_i^2 + 1)
        sig[-1] = 0.0
        up, down = plan[:, 9], plan[:, 5] + sig[:-1]                                # c_noise = sigma_up, c0 = sigma_down - sigma_i
        assert np.abs(up ** 2 + down ** 2 - sig[1:] ** 2).max() < 1e-10 * max(1.0, sig[0] ** 2)
        var = sig[0] ** 2 + 1.0
        assert abs(var - sch.init_noise_sigma ** 2) < 1e-9
        for i in range(n):
            var = (1.0 + plan[i, 5] * sig[i] / (S * S + sig[i] ** 2)) ** 2 * var + plan[i, 9] ** 2
        final.append(var)
    print(f"Euler-ancestral stationary variance at n = 250 / 1000: {final[0]:.4f} / {final[1]:.4f} (s^2 = {S * S})")
    assert final[0] < final[1] and abs(final[1] - S * S) < 0.005


# ------------------------------------------------------------------------------------------------ 5. plan == step
@pytest.mark.parametrize("spacing", ["leading", "trailing"])
@pytest.mark.parametrize("cls", CLASSES, ids=lambda c: c.__name__)
def test_engine_plan_is_the_step_loop(cls, spacing):
    n = 6
    sch = cls(timestep_spacing=spacing)
    sch.set_timesteps(n)
    plan = sch.engine_plan()
    evals = 2 * n - 1 if cls is HeunDiscreteScheduler else n
    assert plan.shape == (evals, PLAN_COLS) and plan.dtype == np.float64 and len(sch.timesteps) == evals
    assert plan[:, 0].tolist() == [float(t) for t in sch.timesteps] and sch.order == (2 if cls is HeunDiscreteScheduler else 1)
    pushes = {EulerDiscreteScheduler: 0, EulerAncestralDiscreteScheduler: 0, HeunDiscreteScheduler: n, DPMSolverMultistepScheduler: n}[cls]
    assert int(plan[:, 10].sum()) == pushes
    assert (plan[:, 9] != 0).sum() == (n - 1 if cls is EulerAncestralDiscreteScheduler else 0)   # the last sigma_up is 0
    # the ancestral step draws one [3] vector per step from g; the same calls on a second generator pre-draw them for the plan
    g, g2 = torch.Generator().manual_seed(11), torch.Generator().manual_seed(11)
    drawn = torch.stack([torch.randn(3, generator=g2, dtype=torch.float64) for _ in range(evals)])
    want = run_steps(sch, n, X_T, gaussian_eps, generator=g if cls is EulerAncestralDiscreteScheduler else None)
    got = run_plan(sch, n, X_T, gaussian_eps, noise=drawn.numpy())
    err = float((got - want).abs().max())
    print(f"{cls.__name__} [{spacing}]: plan vs step loop {err:.2e}")
    assert err < 1e-12


@pytest.mark.parametrize("cls", CLASSES, ids=lambda c: c.__name__)
def test_steps_offset_shifts_the_leading_timesteps(cls):
    """steps_offset = 1 (the usual diffusers configuration value): construction builds no chain, so the offset only has to fit the
    chain that set_timesteps asks for; 50 leading steps are 981, 961, ..., 1, and the table still is the step loop."""
    n = 50
    sch = cls(steps_offset=1)
    assert sch.timesteps.tolist() == list(range(999, -1, -1))              # before set_timesteps: every trained timestep
    with pytest.raises(ValueError):
        sch.engine_plan()
    sch.set_timesteps(n)
    want_ts = [981 - 20 * i for i in range(n)]
    assert want_ts[-1] == 1
    if cls is HeunDiscreteScheduler:
        want_ts = [want_ts[0]] + [t for t in want_ts[1:] for _ in range(2)]
    assert sch.timesteps.tolist() == want_ts and sch.engine_plan()[:, 0].tolist() == [float(t) for t in want_ts]
    g, g2 = torch.Generator().manual_seed(5), torch.Generator().manual_seed(5)
    drawn = torch.stack([torch.randn(3, generator=g2, dtype=torch.float64) for _ in range(len(want_ts))])
    want = run_steps(sch, n, X_T, gaussian_eps, generator=g if cls is EulerAncestralDiscreteScheduler else None)
    got = run_plan(sch, n, X_T, gaussian_eps, noise=drawn.numpy())
    assert float((got - want).abs().max()) < 1e-12
    with pytest.raises(ValueError):
        cls(steps_offset=20).set_timesteps(50)                             # 1000 leaves the trained range


def test_linspace_spacing_is_refused():
    for cls in CLASSES:
        with pytest.raises(ValueError, match="int64"):
            cls(timestep_spacing="linspace")
    with pytest.raises(ValueError):
        DPMSolverMultistepScheduler(solver_order=3)
    with pytest.raises(ValueError):
        DPMSolverMultistepScheduler(lower_order_final=False)
    assert latte_amd.HeunDiscreteScheduler is HeunDiscreteScheduler and latte_amd.DDIMScheduler is DDIMScheduler
    s = EulerDiscreteScheduler(timestep_spacing="trailing")
    s.set_timesteps(4)
    assert s.timesteps.tolist() == [999, 749, 499, 249]


# ================================================================================================ GPU
def _linear_step_reference(x, mo, h, noise, b, C, Cout, F, hw, scale, co):
    """fp64 formula of the step kernel + S, the sum of the absolute values of every product in it (the rounding bound's scale)."""
    m_x, m_eps, c_x, c0, c1, c2, c3, c_noise = [float(np.float32(v)) for v in co]
    scale = float(np.float32(scale))
    mo5 = mo.astype(np.float64).reshape(2 * b, F, Cout, hw)[:, :, :C].transpose(0, 2, 1, 3)      # [2b, C, F, hw]
    un, tx = mo5[:b], mo5[b:]
    x = x.astype(np.float64)
    sd = scale * (tx - un)
    eps = un + sd
    m0 = m_x * x + m_eps * eps
    m0_abs = np.abs(sd) + np.abs(m_x * x) + np.abs(m_eps * eps)
    new = c_x * x + c0 * m0
    tot = m0_abs + np.abs(c_x * x) + np.abs(c0 * m0)
    for cj, hj in zip((c1, c2, c3, c_noise), list(h) + [noise]):
        if cj != 0.0:
            new = new + cj * hj.astype(np.float64)
            tot = tot + np.abs(cj * hj.astype(np.float64))
    return new, m0, tot, m0_abs


STEP_ROWS = {
    # m_x, m_eps, c_x, c0, c1, c2, c3, c_noise | in_scale_next, push, null unused pointers, hw aliased to h3, x_in == x
    "all_ten": ((0.9, -0.4, 0.8, -1.3, 0.6, -0.5, 0.3, 0.7), 0.37, 1, False, False, False),
    "null_history": ((1.1, -0.6, 0.7, 0.45, 0.0, 0.0, 0.0, 0.0), 0.81, 1, True, False, False),
    "alias_h3": ((0.9, -0.4, 0.8, -1.3, 0.6, -0.5, 0.3, 0.7), 0.37, 1, False, True, False),
    "no_push_in_place": ((0.0, 1.0, 1.0, -2.5, 1.25, 0.0, 0.0, 0.0), 1.0, 0, False, False, True),
}


@pytest.mark.gpu
@pytest.mark.parametrize("row", list(STEP_ROWS))
@pytest.mark.parametrize("hw", [25, 64])
@pytest.mark.parametrize("Cout", [4, 8])
def test_linear_step_kernel_matches_fp64_formula(Cout, hw, row):
    from latte_amd._lib import check, load_library, ptr, stream_ptr
    co, in_next, push, nulls, alias, in_place = STEP_ROWS[row]
    b, C, F, scale = 2, 4, 3, 4.5
    g = torch.Generator().manual_seed(3)
    x = torch.randn(b, C, F, hw, generator=g)
    mo = torch.randn(2 * b * F, Cout, hw, generator=g)
    h = [torch.randn(b, C, F, hw, generator=g) for _ in range(3)]
    noise = torch.randn(b, C, F, hw, generator=g)
    want, m0, tot, m0_abs = _linear_step_reference(x.numpy(), mo.numpy(), [t.numpy() for t in h], noise.numpy(), b, C, Cout, F, hw, scale, co)
    dx, dmo, dn = x.cuda(), mo.cuda(), noise.cuda()
    dh = [t.cuda() for t in h]
    dxin = dx if in_place else torch.full_like(dx, 7.0)
    dw = dh[2] if alias else torch.full_like(dx, 7.0)
    args = [None if (nulls and co[4 + j] == 0.0) else dh[j] for j in range(3)] + [None if (nulls and co[7] == 0.0) else dn]
    check(load_library().latte_debug_t2v_linear_step(ptr(dx), ptr(dxin), ptr(dmo), *[ptr(a) for a in args], ptr(dw) if (push or not nulls) else None,
                                                     b, C, Cout, F, hw, scale, *co, in_next, push, stream_ptr()))
    torch.cuda.synchronize()
    bound = 2e-6 * tot
    err = np.abs(dx.cpu().numpy().astype(np.float64) - want)
    print(f"linear step [{row}, Cout {Cout}, hw {hw}]: max |err| / bound = {float((err / bound).max()):.3f}")
    assert (err <= bound).all()
    if not in_place:                                       # x_in = in_scale_next * x' (one more product, of the fp32 x')
        got_in = dxin.cpu().numpy().astype(np.float64)
        assert (np.abs(got_in - float(np.float32(in_next)) * want) <= abs(in_next) * bound + 2e-6 * np.abs(in_next * want)).all()
    if push:
        assert (np.abs(dw.cpu().numpy().astype(np.float64) - m0) <= 2e-6 * m0_abs).all()
    else:
        assert torch.equal(dw.cpu(), torch.full_like(x, 7.0))
    for j in range(3):                                     # the remembered outputs are read only (but for the aliased slot)
        if not (alias and j == 2):
            assert torch.equal(dh[j].cpu(), h[j])
    assert torch.equal(dmo.cpu(), mo) and torch.equal(dn.cpu(), noise)   # the variance channels among them


def _fixture():
    from oracle import latte_t2v_oracle as to
    z = np.load(os.path.join(GOLDEN, "tiny_t2v.npz"))
    cfg = to.T2VConfig(**json.loads(bytes(z["cfg_json"]).decode()))
    sd = {k[4:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd::")}
    return cfg, sd


def _model(cfg, sd, **kw):
    m = latte_amd.LatteT2V(num_attention_heads=cfg.num_attention_heads, attention_head_dim=cfg.attention_head_dim,
                           in_channels=cfg.in_channels, out_channels=cfg.out_channels, num_layers=cfg.num_layers,
                           sample_size=cfg.sample_size, patch_size=cfg.patch_size, cross_attention_dim=cfg.cross_attention_dim,
                           caption_channels=cfg.caption_channels, video_length=cfg.video_length, compute_dtype="f16", **kw)
    m.load_state_dict(sd)
    return m


@pytest.fixture(scope="module")
def t2v_pipe():
    """One engine (max_batch 4) shared by the chain tests; the scheduler is swapped per test."""
    cfg, sd = _fixture()
    pipe = latte_amd.LattePipeline(transformer=_model(cfg, sd, max_batch=4), scheduler=DDIMScheduler()).to("cuda")
    return cfg, sd, pipe


@pytest.mark.gpu
@pytest.mark.parametrize("cls", CLASSES, ids=lambda c: c.__name__)
def test_fused_chain_matches_step_by_step_loop(cls, t2v_pipe):
    cfg, sd, pipe = t2v_pipe
    g = torch.Generator("cpu").manual_seed(9)
    pe, ne = torch.randn(2, 6, cfg.caption_channels, generator=g), torch.randn(2, 6, cfg.caption_channels, generator=g)
    lat = torch.randn(2, 4, cfg.video_length, cfg.sample_size, cfg.sample_size, generator=g)
    pipe.scheduler = cls()
    out, calls = {}, {True: 0, False: 0}
    tr = pipe.transformer
    for fused in (True, False):
        pipe.allow_fused_loop = fused

        def spy(*a, _fused=fused, **kw):
            calls[_fused] += 1
            return type(tr).guided_linear_loop(tr, *a, **kw)

        tr.guided_linear_loop = spy
        try:
            out[fused] = pipe(prompt_embeds=pe, negative_prompt_embeds=ne, num_inference_steps=6, guidance_scale=4.5, latents=lat,
                              generator=torch.Generator("cpu").manual_seed(21), output_type="latents").video
        finally:
            del tr.guided_linear_loop
    pipe.allow_fused_loop = True
    assert calls == {True: 1, False: 0}                     # the fused run is ONE engine call, the other never enters it
    err = rel_l2(out[True], out[False])
    print(f"{cls.__name__}: fused chain vs step-by-step loop rel-L2 {err:.3e}")
    assert torch.isfinite(out[True]).all() and err < 1e-5


@pytest.mark.gpu
def test_chains_match_the_oracle_denoiser_loop(t2v_pipe):
    from oracle import latte_t2v_oracle as to
    cfg, sd, pipe = t2v_pipe
    g = torch.Generator("cpu").manual_seed(9)
    pe, ne = torch.randn(1, 6, cfg.caption_channels, generator=g), torch.randn(1, 6, cfg.caption_channels, generator=g)
    lat = torch.randn(1, 4, cfg.video_length, cfg.sample_size, cfg.sample_size, generator=g)
    steps, scale = 4, 4.5
    pipe.allow_fused_loop = True
    got = {}
    for cls in CLASSES + [DDIMScheduler]:
        pipe.scheduler = cls()
        got[cls] = pipe(prompt_embeds=pe, negative_prompt_embeds=ne, num_inference_steps=steps, guidance_scale=scale, latents=lat,
                        generator=torch.Generator("cpu").manual_seed(21), output_type="latents").video
    for cls in CLASSES:
        sch = cls()
        sch.set_timesteps(steps)
        gen = torch.Generator("cpu").manual_seed(21)
        want = lat.clone() * sch.init_noise_sigma
        with torch.no_grad():
            for t in sch.timesteps:
                x2 = sch.scale_model_input(torch.cat([want] * 2), t)
                out = to.latte_t2v_forward(sd, cfg, x2, t.reshape(1).expand(2), torch.cat([ne, pe]))
                unc, txt = out.chunk(2)
                eps = (unc + scale * (txt - unc)).chunk(2, dim=1)[0]
                want = sch.step(eps, t, want, generator=gen, return_dict=False)[0]
        err = rel_l2(got[cls], want)
        print(f"{cls.__name__}: engine chain vs oracle loop rel-L2 {err:.3e}")
        assert err < 1e-3
    err = rel_l2(got[EulerDiscreteScheduler], got[DDIMScheduler])          # the same ODE step
    print(f"Euler vs DDIM pipeline latents rel-L2 {err:.3e}")
    assert err < 1e-3


@pytest.mark.gpu
def test_linear_loop_argument_checks(t2v_pipe):
    """Every refusal comes from the host checks in front of the first launch: the latents are untouched."""
    from latte_amd._lib import load_library, ptr, stream_ptr
    cfg, sd, pipe = t2v_pipe
    m, lib = pipe.transformer, load_library()
    g = torch.Generator("cpu").manual_seed(1)
    emb = torch.randn(2, 6, cfg.caption_channels, generator=g)
    lat = torch.randn(1, 4, cfg.video_length, cfg.sample_size, cfg.sample_size, generator=g).cuda()
    keep = lat.clone()
    sch = EulerAncestralDiscreteScheduler()
    sch.set_timesteps(3)
    good = sch.engine_plan()
    noise = torch.zeros(3, *lat.shape).cuda()

    def call(plan, samples=1, nz=noise, x=lat):
        plan = np.ascontiguousarray(plan, dtype=np.float64)
        return lib.latte_t2v_guided_linear_loop(m._h, ptr(x), samples, plan.shape[0], plan.ctypes.data, ptr(nz), 4.5, 1, stream_ptr())

    m.set_text(emb)
    assert call(good, nz=None) != 0 and b"c_noise" in lib.latte_last_error()
    bad = good.copy()
    bad[0, 6] = 0.5                                          # c1 on the first row: nothing pushed yet
    assert call(bad) != 0 and b"history" in lib.latte_last_error()
    bad = good.copy()
    bad[1, 5] = float("nan")
    assert call(bad) != 0 and b"non-finite" in lib.latte_last_error()
    bad = good.copy()
    bad[2, 0] = 10.5
    assert call(bad) != 0 and b"integer" in lib.latte_last_error()
    lat3 = torch.zeros(3, *lat.shape[1:]).cuda()
    assert call(good, samples=3, nz=torch.zeros(3, *lat3.shape).cuda(), x=lat3) != 0 and b"max_batch" in lib.latte_last_error()
    m.set_text(emb[:1])                                      # one row installed, the pair needs two
    assert call(good) != 0 and b"text context" in lib.latte_last_error()
    from latte_amd._lib import check
    check(lib.latte_t2v_set_text(m._h, None, None, 0, 0, stream_ptr()))   # uninstalled
    assert call(good) != 0 and b"text context" in lib.latte_last_error()
    torch.cuda.synchronize()
    assert torch.equal(lat, keep)
    with pytest.raises(latte_amd.LatteError):
        m.guided_linear_loop(lat, good[:, :11], None, 4.5)
