"""Euler, Euler-ancestral, Heun and DPM-Solver++(2M) on the class-conditional / unconditional engine: the schedulers on a diffusion's
own timesteps (``set_timesteps(timesteps=, alphas_cumprod_at=)``), the step kernel of this engine's layout (``linear_step_kernel``),
the fused chain ``latte_sample_plan_loop`` and ``SpacedDiffusion.linear_sample_loop``.

What ties the new chains to reference-pinned code: an Euler step in sigma space IS the DDIM eta = 0 step without clipping,
x~' = x~ + (sigma' - sigma) eps with x~ = x / sqrt(abar) -- so over the diffusion's own ``timestep_map`` the Euler chain must reproduce
``ddim_sample_loop``, which tests/test_gpu_parity.py and tests/test_chain250.py hold against chains the reference ran.  On the CPU that is
asserted in fp64 (1e-12); on the engine the two chains feed the denoiser inputs that differ by fp32 rounding only, which f16 operand
rounding re-amplifies: the gap cannot be derived, it is asserted at the project's parity bar (1e-3 relative L2) and recorded.

Figures measured by the GPU tests go into the JSON file LATTE_LINEAR_PARITY_JSON names (-> profiles/linear_sampler_parity.json)."""
import json
import os

import numpy as np
import pytest
import torch

import latte_amd
from latte_amd.schedulers import (PLAN_COLS, DPMSolverMultistepScheduler, EulerAncestralDiscreteScheduler, EulerDiscreteScheduler,
                                  HeunDiscreteScheduler)
from _util import engine_model, load_golden_model, oracle_config, rel_l2

METHODS = ["euler", "euler_a", "heun", "dpmsolver++"]
CLASSES = {"euler": EulerDiscreteScheduler, "euler_a": EulerAncestralDiscreteScheduler, "heun": HeunDiscreteScheduler,
           "dpmsolver++": DPMSolverMultistepScheduler}
KDIFF = ("euler", "euler_a", "heun")
SPECS = ["10", "10,15,20"]          # uniform gaps of 100; the sectioned respacing: 45 timesteps with gaps of 37, 23-24 and 17-18
X_T = np.array([1.3, -0.4, 0.2])
MU = 0.7
TOL = 1e-3                          # the project's parity bar
TOL_PATHS = 1e-4                    # fused loop against the step-by-step loop (tests/test_bpd_loop.py)
INVALID, STATE = 1, 3
_CACHE = {}


def record(key, val):
    path = os.environ.get("LATTE_LINEAR_PARITY_JSON")
    if not path:
        return
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    tab = json.load(open(path)) if os.path.exists(path) else {}
    tab[key] = val
    with open(path, "w") as f:
        json.dump(tab, f, indent=1, sort_keys=True)


def _own(spec):
    """(diffusion, timesteps descending, abar at them) of a respacing."""
    d = latte_amd.create_diffusion(spec)
    return d, d.timestep_map[::-1], d.alphas_cumprod[::-1].copy()


def synthetic_eps(x, t):
    """A smooth eps(x, t) with no structure the samplers could integrate exactly."""
    return 0.5 * np.sin(x + 0.01 * t) + 0.1 * x


def apply_plan(plan, x, model, noise=None, trace=None):
    """The rows of a plan applied in fp64 numpy: the step kernel's formula and the engine's ring of three remembered outputs."""
    hist = [None, None, None]
    for k, (t, in_scale, m_x, m_eps, c_x, c0, c1, c2, c3, c_noise, push, rsv) in enumerate(plan):
        assert t == int(t) and rsv == 0.0 and push in (0.0, 1.0)
        eps = model(in_scale * x, int(t))
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
        if trace is not None:
            trace.append(x.copy())
    return x


# ================================================================================================ CPU
@pytest.mark.parametrize("spec", SPECS)
def test_euler_plan_is_the_fp64_ddim_recursion(spec):
    d, ts, ab = _own(spec)
    n = d.num_timesteps
    assert len(set(np.diff(ts))) > 1 or spec == "10"                      # the sectioned set really has non-uniform gaps
    sch = d.linear_scheduler("euler")
    plan = sch.engine_plan()
    assert plan.shape == (n, PLAN_COLS) and plan[:, 0].tolist() == [float(t) for t in ts]
    got = []
    last = apply_plan(plan, X_T * sch.init_noise_sigma, synthetic_eps, trace=got)
    want, x = [], X_T.copy()
    for i in range(n - 1, -1, -1):                                         # gaussian_diffusion.py:517-564 at eta = 0, unclipped, fp64
        a, ap = d.alphas_cumprod[i], d.alphas_cumprod_prev[i]
        e = synthetic_eps(x, d.timestep_map[i])
        x0 = (x - (1.0 - a) ** 0.5 * e) / a ** 0.5
        x = ap ** 0.5 * x0 + (1.0 - ap) ** 0.5 * e
        want.append(x.copy())
    ab_after = np.append(ab[1:], 1.0)                                      # abar the chain stands at after each step
    err = max(float(np.abs(g * a ** 0.5 - w).max() / np.abs(w).max()) for g, a, w in zip(got, ab_after, want))
    print(f"Euler plan x sqrt(abar) vs fp64 DDIM recursion [{spec}]: {err:.2e}")
    assert err < 1e-12 and float(np.abs(last - want[-1]).max() / np.abs(want[-1]).max()) < 1e-12


def _abar_eps(ts, ab, s):
    """eps* of Gaussian data N(MU, s^2) at the set's timesteps (tests/test_t2v_schedulers.py: gaussian_eps)."""
    at = {int(t): float(a) for t, a in zip(ts, ab)}
    return lambda x, t: (1.0 - at[t]) ** 0.5 * (x - at[t] ** 0.5 * MU) / (at[t] * s * s + 1.0 - at[t])


def _step_loop(sch, x, model, generator=None):
    for t in sch.timesteps:
        eps = torch.from_numpy(model(sch.scale_model_input(x, t).numpy(), int(t)))
        x = sch.step(eps, t, x, return_dict=False, **({"generator": generator} if generator is not None else {}))[0]
    return x


@pytest.mark.parametrize("spec", SPECS)
@pytest.mark.parametrize("method", METHODS)
def test_engine_plan_is_the_step_loop_on_own_timesteps(method, spec):
    d, ts, ab = _own(spec)
    n = len(ts)
    sch = CLASSES[method]()
    sch.set_timesteps(timesteps=ts, alphas_cumprod_at=ab)
    evals = 2 * n - 1 if method == "heun" else n
    plan = sch.engine_plan()
    assert plan.shape == (evals, PLAN_COLS) and len(sch.timesteps) == evals and sch.num_inference_steps == n
    assert plan[:, 0].tolist() == [float(t) for t in sch.timesteps] and np.isfinite(plan).all()
    assert sorted(set(sch.timesteps.tolist()), reverse=True) == list(ts)
    model = _abar_eps(ts, ab, 0.5)
    x0 = torch.from_numpy(X_T * (sch.init_noise_sigma if method in KDIFF else 1.0))
    g, g2 = torch.Generator().manual_seed(11), torch.Generator().manual_seed(11)
    drawn = torch.stack([torch.randn(3, generator=g2, dtype=torch.float64) for _ in range(evals)]).numpy()
    want = _step_loop(sch, x0.clone(), model, generator=g if method == "euler_a" else None).numpy()
    got = apply_plan(plan, x0.numpy().copy(), model, noise=drawn)
    err = float(np.abs(got - want).max())
    print(f"{method} [{spec}]: plan vs step loop {err:.2e}")
    assert err < 1e-12
    # the caller's draw in place of the generator gives the same step
    sch.set_timesteps(timesteps=ts, alphas_cumprod_at=ab)
    x = x0.clone()
    for k, t in enumerate(sch.timesteps):
        eps = torch.from_numpy(model(sch.scale_model_input(x, t).numpy(), int(t)))
        x = sch.step(eps, t, x, return_dict=False, noise=torch.from_numpy(drawn[k]))[0]
    assert float(np.abs(x.numpy() - want).max()) < 1e-12


def test_dpm2m_returns_the_mean_of_a_point_mass_on_non_uniform_timesteps():
    d, ts, ab = _own("10,15,20")
    sch = DPMSolverMultistepScheduler()
    sch.set_timesteps(timesteps=ts, alphas_cumprod_at=ab)
    got = _step_loop(sch, torch.from_numpy(X_T.copy()), _abar_eps(ts, ab, 0.0)).numpy()
    err = float(np.abs(got - MU).max())
    print(f"DPM++ 2M, point mass, 45 non-uniform timesteps: {err:.2e}")
    assert err < 1e-12
    assert (sch.engine_plan()[1:-1, 6] != 0).all()                        # ... through second-order rows, whose r_0 is not 1 here
    lam = np.log(ab ** 0.5) - np.log((1.0 - ab) ** 0.5)
    assert np.ptp(np.diff(lam)[1:] / np.diff(lam)[:-1]) > 0.1


@pytest.mark.parametrize("cls", list(CLASSES.values()), ids=METHODS)
def test_own_timesteps_refusals(cls):
    sch = cls()
    good_t, good_a = [900, 500, 100], [0.1, 0.5, 0.9]
    sch.set_timesteps(timesteps=good_t, alphas_cumprod_at=good_a)
    assert sch.timesteps[0] == 900 and sch.num_inference_steps == 3
    bad = [([100, 500, 900], good_a),            # ascending
           ([900, 500, 500], good_a),            # repeated
           ([900, 100, 500], good_a),            # not monotone
           (good_t, [0.1, 0.5]),                 # length mismatch
           (good_t, [0.1, 0.5, 0.9, 0.95]),
           (good_t, [0.0, 0.5, 0.9]),            # abar outside (0, 1]
           (good_t, [0.1, 0.5, 1.5]),
           (good_t, [-0.1, 0.5, 0.9]),
           (good_t, [0.1, float("nan"), 0.9]),
           ([900, 500.5, 100], good_a),          # not integers
           ([900, 500, -1], good_a),
           (good_t, None), (None, good_a)]       # one without the other
    for t, a in bad:
        with pytest.raises(ValueError):
            sch.set_timesteps(timesteps=t, alphas_cumprod_at=a)
    with pytest.raises(ValueError):
        sch.set_timesteps(4, timesteps=good_t, alphas_cumprod_at=good_a)
    sch.set_timesteps(5)                                                   # the existing call keeps its meaning
    assert sch.timesteps[0] == 800


def test_linear_scheduler_of_a_diffusion_and_its_refusals():
    d = latte_amd.create_diffusion("20")
    for method in METHODS:
        sch = d.linear_scheduler(method)
        assert isinstance(sch, CLASSES[method]) and sch.num_inference_steps == 20
        assert sch.engine_plan().shape[0] == (39 if method == "heun" else 20)
        assert sch.timesteps[0] == d.timestep_map[-1] and sch.timesteps[-1] == d.timestep_map[0]
    assert sorted(latte_amd.LINEAR_METHODS) == sorted(METHODS)
    with pytest.raises(latte_amd.LatteError, match="method"):
        d.linear_scheduler("dpm")
    with pytest.raises(latte_amd.LatteError, match="predict_xstart"):
        latte_amd.create_diffusion("20", predict_xstart=True).linear_scheduler("euler")
    with pytest.raises(latte_amd.LatteError, match="method"):
        d.linear_sample_loop(lambda x, t: x, (1, 4, 4, 8, 8), method="ddim")


# ================================================================================================ GPU: the step kernel
def _step_reference(x, mo, h, noise, B, C, guided, scale, co):
    """fp64 formula of linear_step_kernel on x [B, F, C, hw], mo [B, F, Cout, hw] + the sum of the absolute values of every product in
    it (the rounding bound's scale), as tests/test_t2v_schedulers.py: _linear_step_reference."""
    m_x, m_eps, c_x, c0, c1, c2, c3, c_noise = [float(np.float32(v)) for v in co]
    e = mo.astype(np.float64)[:, :, :C]
    x = x.astype(np.float64)
    if guided:
        hb = B // 2
        cond, unc = e[:hb], e[hb:]
        sd = float(np.float32(scale)) * (cond - unc)
        half = unc + sd
        eps, sd_abs = np.concatenate([half, half]), np.concatenate([np.abs(sd)] * 2)
    else:
        eps, sd_abs = e, 0.0
    m0 = m_x * x + m_eps * eps
    m0_abs = sd_abs + np.abs(m_x * x) + np.abs(m_eps * eps)
    new = c_x * x + c0 * m0
    tot = m0_abs + np.abs(c_x * x) + np.abs(c0 * m0)
    for cj, hj in zip((c1, c2, c3, c_noise), list(h) + [noise]):
        if cj != 0.0:
            new = new + cj * hj.astype(np.float64)
            tot = tot + np.abs(cj * hj.astype(np.float64))
    return new, m0, tot, m0_abs


STEP_ROWS = {
    # m_x, m_eps, c_x, c0, c1, c2, c3, c_noise | in_scale_next, push, null unused pointers, hist_write aliased to h3, x_in == x
    "all_ten": ((0.9, -0.4, 0.8, -1.3, 0.6, -0.5, 0.3, 0.7), 0.37, 1, False, False, False),
    "null_history": ((1.1, -0.6, 0.7, 0.45, 0.0, 0.0, 0.0, 0.0), 0.81, 1, True, False, False),
    "alias_h3": ((0.9, -0.4, 0.8, -1.3, 0.6, -0.5, 0.3, 0.7), 0.37, 1, False, True, False),
    "no_push_in_place": ((0.0, 1.0, 1.0, -2.5, 1.25, 0.0, 0.0, 0.0), 1.0, 0, False, False, True),
}
# one pass of the launch grid is 4096 blocks x 256 threads x 4 floats = 4 194 304 elements: the last case takes a second pass
STEP_SHAPES = [(True, 2, 3), (True, 4, 3), (False, 3, 3)]


def _run_step_case(row, guided, B, F, Cout, hw):
    from latte_amd._lib import check, load_library, ptr, stream_ptr
    co, in_next, push, nulls, alias, in_place = STEP_ROWS[row]
    C, scale = 4, 4.5
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, F, C, hw, generator=g)
    mo = torch.randn(B, F, Cout, hw, generator=g)
    h = [torch.randn(B, F, C, hw, generator=g) for _ in range(3)]
    noise = torch.randn(B, F, C, hw, generator=g)
    want, m0, tot, m0_abs = _step_reference(x.numpy(), mo.numpy(), [t.numpy() for t in h], noise.numpy(), B, C, guided, scale, co)
    dx, dmo, dn = x.cuda(), mo.cuda(), noise.cuda()
    dh = [t.cuda() for t in h]
    dxin = dx if in_place else torch.full_like(dx, 7.0)
    dw = dh[2] if alias else torch.full_like(dx, 7.0)
    args = [None if (nulls and co[4 + j] == 0.0) else dh[j] for j in range(3)] + [None if (nulls and co[7] == 0.0) else dn]
    check(load_library().latte_debug_linear_step(ptr(dx), ptr(dxin), ptr(dmo), *[ptr(a) for a in args], ptr(dw) if (push or not nulls) else None,
                                                 B, C, Cout, F, hw, int(guided), scale, *co, in_next, push, stream_ptr()))
    torch.cuda.synchronize()
    bound = 2e-6 * tot
    err = np.abs(dx.cpu().numpy().astype(np.float64) - want)
    print(f"linear step [{row}, guided {guided}, B {B}, Cout {Cout}, hw {hw}]: max |err| / bound = {float((err / bound).max()):.3f}")
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


@pytest.mark.gpu
@pytest.mark.parametrize("row", list(STEP_ROWS))
@pytest.mark.parametrize("hw", [4, 36])
@pytest.mark.parametrize("Cout", [4, 8])
@pytest.mark.parametrize("guided,B,F", STEP_SHAPES, ids=["guided2", "guided4", "plain3"])
def test_linear_step_kernel_matches_fp64_formula(guided, B, F, Cout, hw, row):
    _run_step_case(row, guided, B, F, Cout, hw)


@pytest.mark.gpu
def test_linear_step_kernel_second_pass_of_the_grid():
    """B F C hw = 2 x 4 x 4 x 140 000 = 4.48 M elements: more than the 4 194 304 one pass of the capped grid covers."""
    assert 2 * 4 * 4 * 140000 > 4096 * 256 * 4
    _run_step_case("alias_h3", True, 2, 4, 8, 140000)


@pytest.mark.gpu
def test_linear_step_kernel_refusals():
    from latte_amd._lib import load_library, ptr, stream_ptr
    lib = load_library()
    x = torch.zeros(2, 3, 4, 36).cuda()
    keep = x.clone()
    mo = torch.ones(2, 3, 8, 36).cuda()

    def call(B=2, C=4, Cout=8, hw=36, guided=1, xx=x, c1=0.0):
        return lib.latte_debug_linear_step(ptr(xx), ptr(xx), ptr(mo), None, None, None, None, None, B, C, Cout, 3, hw, guided, 4.5,
                                           0.0, 1.0, 1.0, 0.5, c1, 0.0, 0.0, 0.0, 1.0, 0, stream_ptr())

    assert call(hw=6) == INVALID and b"multiple of 4" in lib.latte_last_error()
    assert call(B=1) == INVALID and b"doubled batch" in lib.latte_last_error()
    assert call(Cout=6) == INVALID and b"Cout" in lib.latte_last_error()
    assert call(c1=0.5) == INVALID and b"NULL" in lib.latte_last_error()
    assert call(xx=x.view(-1)[1:]) == INVALID and b"aligned" in lib.latte_last_error()
    torch.cuda.synchronize()
    assert torch.equal(x, keep)


# ================================================================================================ GPU: the chains
def _fixture(name):
    """-> (kw, sd, model on the GPU with max_batch 4, latents, model_kwargs, model callable name); one engine per fixture for the module."""
    if name not in _CACHE:
        kw, sd, r = load_golden_model(name)
        m = engine_model(kw, sd, "f16", max_batch=4)
        g = torch.Generator().manual_seed(17)
        z = torch.randn(2, kw["num_frames"], 4, kw["input_size"], kw["input_size"], generator=g)
        if kw["extras"] == 2:                              # guided: the doubled batch with the null class, sample.py:86-94
            z = torch.cat([z, z])
            mk = dict(y=torch.tensor([1, 3, kw["num_classes"], kw["num_classes"]]).cuda(), cfg_scale=4.0)
        else:
            mk = {}
        _CACHE[name] = (kw, sd, m, z.cuda(), mk)
    return _CACHE[name]


def _fn(m, guided):
    return m.forward_with_cfg if guided else m.forward


def _plain(m, guided):
    """The same model behind a plain function: linear_sample_loop then drives it step by step."""
    return (lambda x, t, **k: m.forward_with_cfg(x, t, **k)) if guided else (lambda x, t, **k: m.forward(x, t, **k))


def _step_noise(d, method, z, seed=5):
    n = d.linear_scheduler(method).engine_plan().shape[0]
    return torch.randn((n,) + tuple(z.shape), generator=torch.Generator().manual_seed(seed)).cuda()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tiny_classcond", "tiny_uncond"])
def test_euler_chain_is_the_ddim_chain_on_the_engine(name):
    kw, sd, m, z, mk = _fixture(name)
    guided = kw["extras"] == 2
    d = latte_amd.create_diffusion("10")
    want = d.ddim_sample_loop(_fn(m, guided), z.shape, z, clip_denoised=False, model_kwargs=mk, eta=0.0)
    got = d.linear_sample_loop(_fn(m, guided), z.shape, z, method="euler", model_kwargs=mk)
    err = rel_l2(got, want)
    print(f"Euler vs DDIM(eta = 0, unclipped) on the engine [{name}, f16, create_diffusion('10')]: rel-L2 {err:.3e}")
    record(f"euler_vs_ddim::{name}::f16::10", err)
    assert torch.isfinite(got).all() and err < TOL
    if guided:
        assert torch.equal(got[:2], got[2:])               # the halves of the doubled batch stay bit-identical


@pytest.mark.gpu
def test_chains_match_the_oracle_denoiser_loop():
    """create_diffusion("6"): 6 evaluations (11 for Heun, whose count is always odd), guided at 4.0, the draws given to both sides."""
    from oracle import latte_oracle as lo
    kw, sd, m, z, mk = _fixture("tiny_classcond")
    cfg = oracle_config(kw)
    d = latte_amd.create_diffusion("6")
    y, scale = mk["y"].cpu(), mk["cfg_scale"]
    for method in METHODS:
        nz = _step_noise(d, method, z)
        got = d.linear_sample_loop(m.forward_with_cfg, z.shape, z, method=method, model_kwargs=mk, step_noise=nz)
        sch = d.linear_scheduler(method)
        assert len(sch.timesteps) == (11 if method == "heun" else 6)
        want = z.cpu() * sch.init_noise_sigma
        with torch.no_grad():
            for k, t in enumerate(sch.timesteps):
                tt = torch.full((4,), int(t), dtype=torch.int64)
                out = lo.latte_forward_with_cfg(sd, cfg, sch.scale_model_input(want, t), tt, y, scale)
                want = sch.step(out[:, :, :4], t, want, return_dict=False, noise=nz[k].cpu())[0]      # the learned-sigma half dropped
        err = rel_l2(got, want)
        print(f"{method}: engine chain vs oracle loop rel-L2 {err:.3e}")
        record(f"oracle::{method}::tiny_classcond::f16::6", err)
        assert err < TOL


def _count(monkeypatch, lib, names):
    calls = {n: 0 for n in names}
    for n in names:
        real = getattr(lib, n)

        def wrapper(*a, _real=real, _n=n):
            calls[_n] += 1
            return _real(*a)
        monkeypatch.setattr(lib, n, wrapper, raising=False)
    return calls


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tiny_classcond", "tiny_uncond"])
@pytest.mark.parametrize("method", METHODS)
def test_fused_chain_matches_step_by_step_path(monkeypatch, method, name):
    from latte_amd._lib import load_library
    lib = load_library()
    kw, sd, m, z, mk = _fixture(name)
    guided = kw["extras"] == 2
    d = latte_amd.create_diffusion("6")
    nz = _step_noise(d, method, z)
    evals = nz.shape[0]
    fwd = "latte_forward_with_cfg" if guided else "latte_forward"
    calls = _count(monkeypatch, lib, ["latte_sample_plan_loop", "latte_forward", "latte_forward_with_cfg"])
    fused = d.linear_sample_loop(_fn(m, guided), z.shape, z, method=method, model_kwargs=mk, step_noise=nz)
    assert calls == {**{k: 0 for k in calls}, "latte_sample_plan_loop": 1}, calls      # the fused run is ONE engine call
    for k in calls:
        calls[k] = 0
    stepped = d.linear_sample_loop(_plain(m, guided), z.shape, z, method=method, model_kwargs=mk, step_noise=nz)
    assert calls == {**{k: 0 for k in calls}, fwd: evals}, calls
    err = rel_l2(fused, stepped)
    print(f"{method} [{name}]: fused chain vs step-by-step path rel-L2 {err:.3e}")
    record(f"fused_vs_stepped::{method}::{name}::f16::6", err)
    assert torch.isfinite(fused).all() and err <= TOL_PATHS


@pytest.mark.gpu
def test_chunk_boundary_heun_79_rows():
    """Heun on create_diffusion("40"), guided batch 4: 79 rows with repeated timesteps across the 64-row conditioning chunk (256 / bu)."""
    kw, sd, m, z, mk = _fixture("tiny_classcond")
    d = latte_amd.create_diffusion("40")
    assert d.linear_scheduler("heun").engine_plan().shape[0] == 79 and 256 // z.shape[0] == 64
    fused = d.linear_sample_loop(m.forward_with_cfg, z.shape, z, method="heun", model_kwargs=mk)
    stepped = d.linear_sample_loop(_plain(m, True), z.shape, z, method="heun", model_kwargs=mk)
    err = rel_l2(fused, stepped)
    print(f"Heun 79 rows: fused chain vs step-by-step path rel-L2 {err:.3e}")
    record("fused_vs_stepped::heun::tiny_classcond::f16::40", err)
    assert torch.isfinite(fused).all() and err <= TOL_PATHS


@pytest.mark.gpu
def test_every_row_is_conditioned_on_its_own_timestep():
    """The golden fixtures barely react to the timestep (t_embedder and the adaLN weights are N(0, 0.02)): conditioning rows 64 ... 78 of
    the chain above on the NEXT row's timestep moves its result by 3e-7, under any bound -- and a chain through a model that does react
    amplifies the last-bit difference between Heun's two forms beyond it (9e-3 over 79 evaluations at adaLN weights N(0, 0.3)).  So the
    row offsets are checked one row at a time, without a chain in between: the two-block shape with adaLN weights N(0, 0.1) and a
    t_embedder ten times larger, a plan of the same 79 Heun timesteps whose rows are x <- eps(x, t_k) (m_eps = c0 = 1, everything else
    0), and every row of the trail against the stand-alone forward_with_cfg on the previous row at t_k, which computes its conditioning
    from t_k alone.  Bound: TOL_PATHS, the fused / step-by-step bar; the same forward at the next row's timestep is shown to differ by
    more than a thousand times that, so a row offset that is one off fails at the first row it touches."""
    from latte_amd._lib import check, load_library, ptr, stream_ptr
    from oracle import latte_oracle as lo
    kw, _, _, z, mk = _fixture("tiny_classcond")
    sd = lo.init_state_dict(oracle_config(kw), seed=3, gate_std=0.1, final_std=0.05)
    for k in ("t_embedder.mlp.0.weight", "t_embedder.mlp.2.weight"):
        sd[k] = sd[k] * 10.0
    m = engine_model(kw, sd, "f16", max_batch=4)
    ts = latte_amd.create_diffusion("40").linear_scheduler("heun").engine_plan()[:, 0]
    n = len(ts)
    assert n == 79 and n > 256 // z.shape[0] and ts[1] == ts[2]                 # past the 64-row chunk, with repeated timesteps
    plan = np.zeros((n, PLAN_COLS))
    plan[:, 0], plan[:, 1], plan[:, 3], plan[:, 5] = ts, 1.0, 1.0, 1.0
    x = z.clone()
    trail = torch.empty((n,) + tuple(z.shape), device="cuda")
    check(load_library().latte_sample_plan_loop(m.engine(4, guided=True), 1, mk["cfg_scale"], ptr(x), ptr(mk["y"]), 4, n, plan.ctypes.data,
                                                None, ptr(trail), stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(trail[-1], x) and torch.isfinite(trail).all()

    def alone(xx, t):
        return m.forward_with_cfg(xx, torch.full((4,), int(t), device="cuda", dtype=torch.int64), **mk)[:, :, :4]

    errs, teeth, prev = [], [], z
    for k in range(n):
        want = alone(prev, ts[k])
        errs.append(rel_l2(trail[k], want))
        if k + 1 < n and ts[k + 1] != ts[k]:
            teeth.append(rel_l2(alone(prev, ts[k + 1]), want))
        prev = trail[k]
    print(f"79 rows, each against the stand-alone forward at its own timestep: worst rel-L2 {max(errs):.3e} (row {int(np.argmax(errs))}); "
          f"the next row's timestep instead: {min(teeth):.3e} ... {max(teeth):.3e}")
    record("rows_vs_standalone_forward::gated_two_block::f16::79", {"worst": max(errs), "next_timestep_instead_min": min(teeth)})
    assert min(teeth) > 1000 * TOL_PATHS and max(errs) <= TOL_PATHS


@pytest.mark.gpu
def test_engine_noise_is_seeded_and_explicit_noise_is_what_the_trail_shows():
    kw, sd, m, z, mk = _fixture("tiny_classcond")
    d = latte_amd.create_diffusion("6")

    def run(seed):
        m.set_engine_option("seed", seed, batch=4, guided=True)
        return d.linear_sample_loop(m.forward_with_cfg, z.shape, z, method="euler_a", model_kwargs=mk).cpu()

    a, b, c = run(5), run(5), run(6)
    assert torch.equal(a, b) and not torch.equal(a, c) and torch.isfinite(c).all()
    # explicit draws: moving row j of step_noise by delta moves the trail from row j on, there by c_noise_j * delta, and nothing before
    plan = d.linear_scheduler("euler_a").engine_plan()
    j = 2
    nz = _step_noise(d, "euler_a", z)
    nz2 = nz.clone()
    delta = torch.randn(z.shape, generator=torch.Generator().manual_seed(8)).cuda()
    nz2[j] += delta
    t1, t2 = ([r["sample"].cpu() for r in d.linear_sample_loop_progressive(m.forward_with_cfg, z.shape, z, method="euler_a",
                                                                           model_kwargs=mk, step_noise=s)] for s in (nz, nz2))
    assert len(t1) == 6 and all(torch.equal(t1[k], t2[k]) for k in range(j)) and not torch.equal(t1[j + 1], t2[j + 1])
    cn = float(np.float32(plan[j, 9]))
    p1, p2 = cn * nz[j].cpu().double(), cn * nz2[j].cpu().double()
    gap = (t2[j].double() - t1[j].double() - (p2 - p1)).abs()       # two fp32 sums that differ in one product
    assert float((gap / (1e-6 * (t1[j].abs().double() + t2[j].abs().double() + p1.abs() + p2.abs()))).max()) <= 1.0
    assert float(plan[5, 9]) == 0.0                        # the last row draws nothing: NULL noise there is legal


@pytest.mark.gpu
def test_trail_ends_at_the_returned_latents():
    for name in ("tiny_classcond", "tiny_uncond"):
        kw, sd, m, z, mk = _fixture(name)
        guided = kw["extras"] == 2
        d = latte_amd.create_diffusion("6")
        for method in ("dpmsolver++", "heun"):
            final = d.linear_sample_loop(_fn(m, guided), z.shape, z, method=method, model_kwargs=mk)
            trail = list(d.linear_sample_loop_progressive(_fn(m, guided), z.shape, z, method=method, model_kwargs=mk))
            assert len(trail) == (11 if method == "heun" else 6)
            assert torch.equal(trail[-1]["sample"], final) and not torch.equal(trail[0]["sample"], final)


@pytest.mark.gpu
def test_plan_loop_argument_checks():
    """Every refusal comes from the host checks in front of the first launch: non-zero, its message, and the latents untouched."""
    from latte_amd._lib import load_library, ptr, stream_ptr
    lib = load_library()
    kw, sd, m, z, mk = _fixture("tiny_classcond")
    d = latte_amd.create_diffusion("6")
    good = d.linear_scheduler("dpmsolver++").engine_plan()
    x = z.clone()
    eng = m.engine(4, guided=True)

    def call(plan, batch=4, guided=1, y=mk["y"], e=eng, xx=x):
        plan = np.ascontiguousarray(plan, dtype=np.float64)
        rc = lib.latte_sample_plan_loop(e, guided, 4.0, ptr(xx), ptr(y), batch, plan.shape[0], plan.ctypes.data, None, None, stream_ptr())
        return rc, lib.latte_last_error()

    def bad(r, c, v):
        p = good.copy()
        p[r, c] = v
        return p

    cases = [(bad(1, 5, float("nan")), {}, INVALID, b"non-finite"),
             (bad(1, 2, float("inf")), {}, INVALID, b"non-finite"),
             (bad(2, 0, 10.5), {}, INVALID, b"integer"),
             (bad(2, 0, -1.0), {}, INVALID, b"integer"),
             (bad(0, 0, 1000.0), {}, INVALID, b"trained range"),
             (bad(0, 6, 0.5), {}, INVALID, b"history"),              # c1 on the first row: nothing pushed yet
             (bad(1, 7, 0.5), {}, INVALID, b"history"),              # c2 after one push
             (bad(1, 10, 2.0), {}, INVALID, b"push"),
             (bad(1, 11, 1.0), {}, INVALID, b"push"),
             (good, dict(batch=m.max_batch + 1), STATE, b"max_batch"),
             (good, dict(batch=3), INVALID, b"doubled batch"),
             (good, dict(y=None), INVALID, b"needs y"),
             (np.repeat(good[:1], 4097, axis=0), {}, INVALID, b"4096 evaluations")]
    for plan, kwargs, code, msg in cases:
        rc, text = call(plan, **kwargs)
        assert rc == code and msg in text, (rc, text, msg)
    torch.cuda.synchronize()
    assert torch.equal(x, z)
    with pytest.raises(latte_amd.LatteError, match="step_noise"):
        d.linear_sample_loop(m.forward_with_cfg, z.shape, z, method="heun", model_kwargs=mk, step_noise=torch.zeros((6,) + tuple(z.shape)))
    # the text-embedding model without its embedding
    kw_t, sd_t, _ = load_golden_model("tiny_textcond")
    mt = engine_model(kw_t, sd_t, "f16", max_batch=2)
    xt = torch.randn(2, kw_t["num_frames"], 4, kw_t["input_size"], kw_t["input_size"]).cuda()
    keep = xt.clone()
    rc, text = call(good, batch=2, guided=0, y=None, e=mt.engine(2), xx=xt)
    assert rc == STATE and b"set_text_embedding" in text, (rc, text)
    torch.cuda.synchronize()
    assert torch.equal(xt, keep)
