"""DDIM inversion end to end: ``SpacedDiffusion.ddim_reverse_sample_loop`` as ONE latte_invert_loop call inside the engine and as the
step-by-step loop over a plain model callable, against tests/golden/invert.npz -- the reference's own ddim_reverse_sample stepped over
create_diffusion("50") on fixture M of tests/bpd_reference.py (a two-block class-conditional Latte, gates N(0, 0.1), B = 2), with
clip_denoised on and off and through forward_with_cfg at scale 4.0 on the doubled batch.

Bounds: f16 operands hold the project's 1e-3 parity bar (relative L2) at every stored checkpoint -- the sample after steps 0, 1, 24,
48, 49 and the last pred_xstart; a 3e-4 perturbation of every model output grows to 3.9e-4 / 1.6e-4 over this chain (clip off / on),
as over the sampling chain.  bf16 operands are recorded and asserted at the bound tests/test_gpu_parity.py gives bf16 at this gate
scale.

The last pred_xstart is NOT held to a relative-L2 bound of its own, and cannot be: at index 49 it is clamp(157.4 x_48 - 157.4 eps), a
157-fold amplified difference of which the clamp keeps the 10 - 16 % of elements that land inside [-1, 1].  Under the 3e-4 perturbation
above, the reference's own last pred_xstart moves by 1.6e-2 (clip on) / 9.0e-3 (clip off) relative L2 while its sample moves by
1.6e-4 / 3.9e-4.  Measured on the engine with f16 operands: 2.3e-3 (clip on) beside 5.2e-5 on the sample.  Since the sample of index
49 IS the re-derived eps (alphas_cumprod_next = 0), the last pred_xstart is a function of the two stored samples 48 and 49, and what is
asserted is exact: element by element it differs from the reference's by no more than those samples' differences explain,
|d x0| <= a |d x_48| + b |d x_49| + fp32 rounding (the clamp is 1-Lipschitz); the figure itself is recorded.  No round trip through an untrained model is asserted anywhere: its sampling chain blows up."""
import os

import numpy as np
import pytest
import torch

import invert_reference as ir
from _util import GOLDEN, engine_model, load_golden_model, rel_l2

pytestmark = pytest.mark.gpu
TOL = 1e-3          # the project's parity bar
TOL_BF16 = 1e-2     # tests/test_gpu_parity.py: BF16_TOL_AT_TRAINED_GATES
TOL_PATHS = 1e-4    # fused loop against the step-by-step loop (tests/test_bpd_loop.py)
T = 50
INVALID, STATE = 1, 3
_CACHE = {}


def _golden():
    return np.load(os.path.join(GOLDEN, "invert.npz"))


def _fixture(case="clip1", extras=2, learn_sigma=True, cd="f16"):
    """-> (diffusion, model on the GPU, model callable, x, model_kwargs, clip_denoised); one engine per variant for the module."""
    import latte_amd
    key = (extras, learn_sigma, cd)
    if key not in _CACHE:
        kw, _, sd, _, _, _ = ir.model_inputs(extras, learn_sigma)
        _CACHE[key] = (latte_amd.create_diffusion(ir.M_SPEC, learn_sigma=learn_sigma), engine_model(kw, sd, cd, max_batch=4))
    d, m = _CACHE[key]
    _, _, _, x, y, guided = ir.model_chain_inputs(case, extras, learn_sigma)
    mk = {} if y is None else dict(y=y.cuda())
    if guided:
        mk["cfg_scale"] = ir.M_CFG_SCALE
    return d, m, (m.forward_with_cfg if guided else m.forward), x.cuda(), mk, ir.model_case(case)[0]


def _fused(case, cd="f16"):
    """The progressive generator on the engine path -> {"sample": [T, B, ...], "pred_xstart": [T, B, ...]} on the host."""
    key = ("fused", case, cd)
    if key not in _CACHE:
        d, m, fn, x, mk, clip = _fixture(case, cd=cd)
        trail = list(d.ddim_reverse_sample_loop_progressive(fn, x, clip_denoised=clip, model_kwargs=mk))
        assert len(trail) == T
        _CACHE[key] = {k: torch.stack([r[k] for r in trail]).cpu() for k in ("sample", "pred_xstart")}
    return _CACHE[key]


X0_ROUNDING = 2e-4   # fp32 rounding of 157.4 x - 157.4 eps at |x|, |eps| <= 4: two products of 630 at 2^-24 each, and their difference


def _errors(got, want):
    """Relative L2 at every stored checkpoint; the last pred_xstart's is measured under "recorded::" (see the module docstring)."""
    err = {f"sample@{k}": rel_l2(got["sample"][k], torch.from_numpy(want["sample"][j])) for j, k in enumerate(ir.M_CHECKPOINTS)}
    err["recorded::pred_xstart@49"] = rel_l2(got["pred_xstart"][-1], torch.from_numpy(want["pred_xstart"]))
    return err


def _check(d, got, want, tol):
    """The samples at ``tol``; the last pred_xstart within what the differences of samples 48 and 49 explain, element by element."""
    err = _errors(got, want)
    assert all(v < tol for k, v in err.items() if k.startswith("sample@")), err
    a, b = np.float32(d.sqrt_recip_alphas_cumprod[T - 1]), np.float32(d.sqrt_recipm1_alphas_cumprod[T - 1])
    assert ir.M_CHECKPOINTS[-2:] == (T - 2, T - 1)
    d48, d49 = ((got["sample"][k] - torch.from_numpy(want["sample"][j])).abs() for j, k in ((-2, T - 2), (-1, T - 1)))
    dx0 = (got["pred_xstart"][-1] - torch.from_numpy(want["pred_xstart"])).abs()
    over = dx0 - (float(a) * d48 + float(b) * d49 + X0_ROUNDING)
    assert float(over.max()) <= 0.0, (float(over.max()), err)
    return err


def _want(case):
    z = _golden()
    return {k: z[f"M::{case}::{k}"] for k in ("sample", "pred_xstart")}


@pytest.mark.parametrize("case", ir.M_CASES)
def test_fused_loop_matches_reference(case):
    got = _fused(case)
    print("f16", case, _errors(got, _want(case)))
    ir.record(f"M::fused::f16::{case}", _errors(got, _want(case)))
    assert torch.isfinite(got["sample"]).all() and torch.isfinite(got["pred_xstart"]).all()
    _check(_fixture(case)[0], got, _want(case), TOL)
    if case == "guided":       # the halves of the doubled batch stay bit-identical
        assert torch.equal(got["sample"][:, :2], got["sample"][:, 2:]) and torch.equal(got["pred_xstart"][:, :2], got["pred_xstart"][:, 2:])
    if case != "clip0":
        assert float(got["pred_xstart"].abs().max()) <= 1.0


@pytest.mark.parametrize("case", ir.M_CASES)
def test_fused_loop_bf16_operands_recorded(case):
    err = _errors(_fused(case, "bf16"), _want(case))
    print("bf16", case, err)
    ir.record(f"M::fused::bf16::{case}", err)
    _check(_fixture(case)[0], _fused(case, "bf16"), _want(case), TOL_BF16)


def _count(monkeypatch, lib, names):
    calls = {n: 0 for n in names}
    for n in names:
        real = getattr(lib, n)

        def wrapper(*a, _real=real, _n=n):
            calls[_n] += 1
            return _real(*a)
        monkeypatch.setattr(lib, n, wrapper, raising=False)
    return calls


def test_engine_path_is_one_call_and_the_callable_path_steps(monkeypatch, lib):
    names = ["latte_invert_loop", "latte_forward", "latte_forward_with_cfg", "latte_sampler_step_ex"]
    calls = _count(monkeypatch, lib, names)
    for case in ir.M_CASES:
        d, m, fn, x, mk, clip = _fixture(case)
        fused = _fused(case)
        for k in calls:
            calls[k] = 0
        x_before = x.clone()
        out = d.ddim_reverse_sample_loop(fn, x, clip_denoised=clip, model_kwargs=mk)
        assert calls == dict.fromkeys(names, 0) | {"latte_invert_loop": 1}, calls
        assert torch.equal(out.cpu(), fused["sample"][-1]) and torch.equal(x, x_before)      # reproducible; the input is not written
        for k in calls:
            calls[k] = 0
        stepped = list(d.ddim_reverse_sample_loop_progressive(lambda xx, tt, **k: fn(xx, tt, **k), x, clip_denoised=clip, model_kwargs=mk))
        fwd = "latte_forward_with_cfg" if case == "guided" else "latte_forward"
        assert calls == dict.fromkeys(names, 0) | {fwd: T, "latte_sampler_step_ex": T}, calls
        stepped = {k: torch.stack([r[k] for r in stepped]).cpu() for k in ("sample", "pred_xstart")}
        err = _errors(stepped, _want(case))
        paths = max(max(rel_l2(stepped[k][j], fused[k][j]) for j in range(T)) for k in ("sample", "pred_xstart"))
        print("stepped", case, err, "fused vs stepped", paths)
        ir.record(f"M::stepped::f16::{case}", err)
        ir.record(f"M::fused_vs_stepped::f16::{case}", paths)
        _check(d, stepped, _want(case), TOL)
        assert paths < TOL_PATHS, paths


def _raw_loop(lib, d, m, x, y, start, end, clip=1, guided=0, scale=1.0, batch=None, trails=True):
    """latte_invert_loop on a copy of x -> (rc, x after, trail_sample, trail_x0), NaN where nothing was written."""
    from latte_amd._lib import ptr, stream_ptr
    B = x.shape[0] if batch is None else batch
    n = max(end - start + 1, 1)
    xx = x.clone()
    ts, t0 = (torch.full((n,) + tuple(x.shape), float("nan"), device="cuda") for _ in range(2)) if trails else (None, None)
    rc = lib.latte_invert_loop(m.engine(x.shape[0], guided=bool(guided)), d._h, clip, guided, scale, ptr(xx), ptr(y), B, start, end, ptr(ts), ptr(t0),
                               stream_ptr())
    torch.cuda.synchronize()
    return rc, xx, ts, t0


def test_split_calls_and_trails(lib):
    d, m, fn, x, mk, clip = _fixture("clip1")
    fused = _fused("clip1")
    # 0 ... 24, then 25 ... 49: the bits of one call, through the public loop
    mid = d.ddim_reverse_sample_loop(fn, x, clip_denoised=clip, model_kwargs=mk, end_index=24)
    assert torch.equal(mid.cpu(), fused["sample"][24])
    end = d.ddim_reverse_sample_loop(fn, mid, clip_denoised=clip, model_kwargs=mk, start_index=25)
    assert torch.equal(end.cpu(), fused["sample"][-1])
    # the trails of the raw call are the progressive generator's values, in execution order; x ends on the last sample
    rc, xx, ts, t0 = _raw_loop(lib, d, m, x, mk["y"], 0, T - 1)
    assert rc == 0, lib.latte_last_error()
    assert torch.equal(ts.cpu(), fused["sample"]) and torch.equal(t0.cpu(), fused["pred_xstart"]) and torch.equal(xx, ts[-1])
    assert not torch.equal(ts[0], ts[1])
    # a single step in the middle, run alone from the trail's value, without trails
    rc, xx, _, _ = _raw_loop(lib, d, m, ts[29].contiguous(), mk["y"], 30, 30, trails=False)
    assert rc == 0 and torch.equal(xx, ts[30])
    # the public single step on the engine's forward
    r = d.ddim_reverse_sample(m.forward, ts[29], torch.full((2,), 30, device="cuda"), clip_denoised=clip, model_kwargs=mk)
    assert rel_l2(r["sample"], ts[30]) < TOL_PATHS and rel_l2(r["pred_xstart"], t0[30]) < TOL_PATHS


def test_partial_ddim_sample_loop_keeps_the_default_chain():
    """start_index / end_index of ddim_sample_loop: the default is the full chain, bit for bit, and two partial calls compose to it."""
    d, m, fn, x, mk, clip = _fixture("clip1")
    full = d.ddim_sample_loop(fn, x.shape, x, clip_denoised=clip, model_kwargs=mk, device="cuda")
    same = d.ddim_sample_loop(fn, x.shape, x, clip_denoised=clip, model_kwargs=mk, device="cuda", start_index=T - 1, end_index=0)
    hi = d.ddim_sample_loop(fn, x.shape, x, clip_denoised=clip, model_kwargs=mk, device="cuda", end_index=20)
    lo = d.ddim_sample_loop(fn, x.shape, hi, clip_denoised=clip, model_kwargs=mk, device="cuda", start_index=19)
    assert torch.equal(full, same) and torch.equal(full, lo) and not torch.equal(full, hi)
    stepped = d.ddim_sample_loop(lambda xx, tt, **k: fn(xx, tt, **k), x.shape, hi, clip_denoised=clip, model_kwargs=mk, device="cuda", start_index=19)
    assert rel_l2(stepped, full) < TOL_PATHS
    from latte_amd import LatteError
    for bad in (dict(start_index=T), dict(start_index=3, end_index=4), dict(end_index=-1)):
        with pytest.raises(LatteError, match="index range"):
            d.ddim_sample_loop(fn, x.shape, x, model_kwargs=mk, device="cuda", **bad)
    for bad in (dict(end_index=T), dict(start_index=4, end_index=3), dict(start_index=-1)):
        with pytest.raises(LatteError, match="index range"):
            d.ddim_reverse_sample_loop(fn, x, model_kwargs=mk, **bad)


def test_full_length_chain_is_finite_and_splits_across_conditioning_chunks():
    """create_diffusion("") -- 1000 steps; at B = 2 the chain conditioning comes in chunks of 128 steps, and 0 ... 299 + 300 ... 999
    starts its second call in the middle of one."""
    import latte_amd
    _, m, fn, x, mk, clip = _fixture("clip1")
    d = latte_amd.create_diffusion("")
    one = d.ddim_reverse_sample_loop(fn, x, clip_denoised=clip, model_kwargs=mk)
    assert torch.isfinite(one).all()
    a = d.ddim_reverse_sample_loop(fn, x, clip_denoised=clip, model_kwargs=mk, end_index=299)
    b = d.ddim_reverse_sample_loop(fn, a, clip_denoised=clip, model_kwargs=mk, start_index=300)
    assert torch.equal(one, b) and not torch.equal(one, a)


@pytest.mark.parametrize("extras,learn_sigma", [(1, True), (2, False)], ids=["unconditional", "fixed_variance"])
def test_other_models_match_the_restatement(extras, learn_sigma):
    d, m, fn, x, mk, clip = _fixture("clip1", extras, learn_sigma)
    want = ir.model_restatement("clip1", extras, learn_sigma)
    trail = list(d.ddim_reverse_sample_loop_progressive(fn, x, clip_denoised=clip, model_kwargs=mk))
    got = {k: torch.stack([r[k] for r in trail]).cpu() for k in ("sample", "pred_xstart")}
    err = _errors(got, want)
    print(extras, learn_sigma, err)
    ir.record(f"M::fused::f16::extras{extras}::learn_sigma{int(learn_sigma)}", err)
    _check(d, got, want, TOL)


def test_the_sampler_noise_stream_is_left_alone(lib):
    from latte_amd._lib import check, ptr, stream_ptr
    d, m, fn, x, mk, clip = _fixture("clip1")

    def sample():     # DDPM steps drawing from the engine's Philox stream (noise = NULL)
        xx = x.clone()
        check(lib.latte_sample_loop(m.engine(2), d._h, 0, 0.0, 1, 1.0, ptr(xx), ptr(mk["y"]), 2, 5, 0, None, None, None, stream_ptr()))
        torch.cuda.synchronize()
        return xx.cpu()

    m.set_engine_option("seed", 9, batch=2)
    s1, s2 = sample(), sample()
    assert not torch.equal(s1, s2)                       # the second loop continues the stream
    m.set_engine_option("seed", 9, batch=2)
    t1 = sample()
    d.ddim_reverse_sample_loop(fn, x, clip_denoised=clip, model_kwargs=mk)      # draws nothing: the Philox offset stays
    t2 = sample()
    assert torch.equal(s1, t1) and torch.equal(s2, t2)


def _untouched(xx, x, ts, t0):
    return torch.equal(xx, x) and bool(torch.isnan(ts).all()) and bool(torch.isnan(t0).all())


def test_refusals(lib):
    import latte_amd
    from latte_amd import LatteError
    d, m, fn, x, mk, clip = _fixture("clip1")
    y = mk["y"]
    for start, end in ((0, T), (4, 3), (-1, 3)):
        rc, xx, ts, t0 = _raw_loop(lib, d, m, x, y, start, end)
        assert rc == INVALID and b"index range" in lib.latte_last_error() and _untouched(xx, x, ts, t0), (start, end)
    rc, xx, ts, t0 = _raw_loop(lib, d, m, x, y, 0, T - 1, batch=m.max_batch + 1)
    assert rc == STATE and b"max_batch" in lib.latte_last_error() and _untouched(xx, x, ts, t0)
    rc, xx, ts, t0 = _raw_loop(lib, latte_amd.create_diffusion(ir.M_SPEC, learn_sigma=False), m, x, y, 0, T - 1)
    assert rc == INVALID and b"learn_sigma" in lib.latte_last_error() and _untouched(xx, x, ts, t0)
    rc, xx, ts, t0 = _raw_loop(lib, d, m, x, None, 0, T - 1)
    assert rc == INVALID and b"needs y" in lib.latte_last_error() and _untouched(xx, x, ts, t0)
    x3 = torch.cat([x, x[:1]]).contiguous()
    rc, xx, ts, t0 = _raw_loop(lib, d, m, x3, torch.cat([y, y[:1]]).contiguous(), 0, T - 1, guided=1, scale=4.0)
    assert rc == INVALID and b"doubled batch" in lib.latte_last_error() and _untouched(xx, x3, ts, t0)
    # a text-conditioned model (extras = 78) without an installed text embedding
    kw, sd, r = load_golden_model("tiny_textcond")
    mt = engine_model(kw, sd, "f16", max_batch=2)
    dt = latte_amd.create_diffusion("50", learn_sigma=kw["learn_sigma"])
    xt = torch.from_numpy(r["x"]).cuda()[:2].contiguous()
    rc, xx, ts, t0 = _raw_loop(lib, dt, mt, xt, None, 0, 3)
    assert rc == STATE and b"set_text_embedding" in lib.latte_last_error() and _untouched(xx, xt, ts, t0)
    # the host interface
    with pytest.raises(LatteError, match="labels y"):
        d.ddim_reverse_sample_loop(fn, x, model_kwargs={})
    with pytest.raises(LatteError, match="learn_sigma"):
        latte_amd.create_diffusion(ir.M_SPEC, learn_sigma=False).ddim_reverse_sample_loop(fn, x, model_kwargs=mk)
