"""The DDIM reverse step one call at a time: latte_sampler_step / latte_sampler_step_ex with method 2 (gaussian_diffusion.py:566-602)
against tests/golden/invert.npz -- what the reference's ddim_reverse_sample computed on the kernel-level fixtures of
tests/invert_reference.py: every ModelMeanType x ModelVarType, clip_denoised on and off, 432 / 1024 / 65 536 elements per sample,
indices {0, 1, 25, 48, 49} of "50" and {0, 999} of "" (T-1 is the alphas_cumprod_next = 0 row, 0 the division by 0.01) -- and against a
model that is consistent with a known (x_0, eps), which needs no reference and catches a wrong `next` index.

Bound: 2e-5 relative L2, the bound tests/test_bpd_kernels.py holds its fp32 kernels to.  The fixture keeps K_KEEP elements and the
sums of every result; the whole tensors are compared with the restatement that tests/test_invert_reference.py pins to the fixture."""
import os

import numpy as np
import pytest
import torch

import invert_reference as ir
from _util import GOLDEN, rel_l2
from oracle import diffusion_oracle as do

pytestmark = pytest.mark.gpu
TOL = 2e-5
INVALID = 1


def _golden():
    return np.load(os.path.join(GOLDEN, "invert.npz"))


def _t(d, index, B):
    return torch.full((B,), index, dtype=torch.int64, device="cuda")


def _reverse(d, mo, x, index, clip, **hooks):
    return d.ddim_reverse_sample(lambda xx, tt, **k: mo, x, _t(d, index, x.shape[0]), clip_denoised=clip, model_kwargs={}, **hooks)


@pytest.mark.parametrize("clip", [True, False], ids=["clip", "noclip"])
@pytest.mark.parametrize("tag", sorted(ir.K_TYPES))
def test_reverse_step_matches_reference(tag, clip):
    import latte_amd
    z = _golden()
    worst = {"sample": 0.0, "pred_xstart": 0.0, "kept": 0.0, "sumsq": 0.0}
    for spec, shape, index in ir.kernel_grid():
        kw = ir.K_TYPES[tag]
        d = latte_amd.create_diffusion(spec, **kw)
        s = do.Schedule(spec, **kw)
        _, _, x_t, mo = ir.kernel_inputs(s, shape, index)
        got = _reverse(d, mo.cuda(), x_t.cuda(), index, clip)
        assert set(got) == {"sample", "pred_xstart"} and all(torch.isfinite(v).all() for v in got.values())
        key = ir.kernel_key(tag, clip, spec, shape, index)
        vals, sums = ir.kernel_digest(got)
        kept = max(rel_l2(torch.from_numpy(vals[j]), torch.from_numpy(z[key][j])) for j in range(2))
        sumsq = ir.rel_max(sums[:, 1], z[key + "::sums"][:, 1])
        want = ir.ddim_reverse_sample(s, mo, x_t, index, clip)
        err = {k: rel_l2(got[k], want[k]) for k in ("sample", "pred_xstart")}
        print(tag, clip, spec, shape, index, err, kept, sumsq)
        worst = {k: max(worst[k], v) for k, v in dict(err, kept=kept, sumsq=sumsq).items()}
        assert kept < TOL and sumsq < TOL and max(err.values()) < TOL, (key, err, kept, sumsq)
        if clip:
            assert float(got["pred_xstart"].abs().max()) <= 1.0
    ir.record(f"kernel::{tag}::clip{int(clip)}", worst)


def _case(tag="eps_learned", spec="50", shape=ir.K_SHAPES[0], index=25):
    import latte_amd
    kw = ir.K_TYPES[tag]
    d, s = latte_amd.create_diffusion(spec, **kw), do.Schedule(spec, **kw)
    _, nz, x_t, mo = ir.kernel_inputs(s, shape, index)
    return d, s, x_t, mo, nz


@pytest.mark.parametrize("tag", ["eps_learned", "xstart_fixed_small"])
def test_hooks_through_step_ex_match_the_restatement(tag):
    worst = 0.0
    for index in (0, 25, 49):
        d, s, x_t, mo, _ = _case(tag, index=index)
        t_orig = torch.full((x_t.shape[0],), s.timestep_map[index], dtype=torch.int64)
        for clip in (True, False):
            for hooks in (dict(denoised_fn=do.example_denoised_fn), dict(cond_fn=do.example_cond_fn),
                          dict(denoised_fn=do.example_denoised_fn, cond_fn=do.example_cond_fn)):
                got = _reverse(d, mo.cuda(), x_t.cuda(), index, clip, **hooks)
                grad = do.example_cond_fn(x_t, t_orig) if "cond_fn" in hooks else None
                want = ir.ddim_reverse_sample(s, mo, x_t, index, clip, hooks.get("denoised_fn"), grad)
                err = max(rel_l2(got[k], want[k]) for k in want)
                worst = max(worst, err)
                assert err < TOL, (tag, index, clip, sorted(hooks), err)
                if index == 25:      # where either hook moves the sample by 2e-3 or more: a hook that was dropped would show
                    assert rel_l2(want["sample"], ir.ddim_reverse_sample(s, mo, x_t, index, clip)["sample"]) > 1e-3
    ir.record(f"kernel::hooks::{tag}", worst)


def _raw(lib, d, method, index, eta, x, mo, noise, sample, x0, predict_only=0, clip=1):
    from latte_amd._lib import ptr, stream_ptr
    B, F, C = x.shape[:3]
    rc = lib.latte_sampler_step_ex(d._h, method, index, eta, clip, ptr(x), ptr(mo), ptr(noise), None, None, predict_only, B, F, C,
                                   x.shape[3] * x.shape[4], ptr(sample), ptr(x0), stream_ptr())
    torch.cuda.synchronize()
    return rc


def test_predict_only_aliasing_noise_and_eta(lib):
    d, s, x_t, mo, nz = _case()
    x, mo_d = x_t.cuda(), mo.cuda()
    want = ir.ddim_reverse_sample(s, mo, x_t, 25, True)
    raw = ir.ddim_reverse_sample(s, mo, x_t, 25, False)["pred_xstart"]         # before the clamp
    assert float(raw.abs().max()) > 1.0
    nan = torch.full_like(x, float("nan"))
    # predict_only: the raw x_start prediction and nothing else
    sample, x0 = nan.clone(), nan.clone()
    assert _raw(lib, d, 2, 25, 0.0, x, mo_d, None, sample, x0, predict_only=1) == 0, lib.latte_last_error()
    assert rel_l2(x0, raw) < TOL and bool(torch.isnan(sample).all())
    # the step proper; noise is ignored (a NaN buffer changes no bit); outputs may alias x
    a_s, a_0 = nan.clone(), nan.clone()
    assert _raw(lib, d, 2, 25, 0.0, x, mo_d, None, a_s, a_0) == 0, lib.latte_last_error()
    b_s, b_0 = nan.clone(), nan.clone()
    assert _raw(lib, d, 2, 25, 0.0, x, mo_d, nan, b_s, b_0) == 0, lib.latte_last_error()
    assert rel_l2(a_s, want["sample"]) < TOL and rel_l2(a_0, want["pred_xstart"]) < TOL
    assert torch.equal(a_s, b_s) and torch.equal(a_0, b_0)
    xa = x.clone()
    assert _raw(lib, d, 2, 25, 0.0, xa, mo_d, None, xa, b_0) == 0, lib.latte_last_error()
    assert torch.equal(xa, a_s)
    from latte_amd._lib import ptr, stream_ptr
    c_s = nan.clone()                                                         # the plain entry point, pred_xstart_out = NULL
    assert lib.latte_sampler_step(d._h, 2, 25, 0.0, 1, ptr(x), ptr(mo_d), None, *x.shape[:3], 36, ptr(c_s), None, stream_ptr()) == 0
    torch.cuda.synchronize()
    assert torch.equal(c_s, a_s)
    # eta != 0: "Reverse ODE only for deterministic path" (gd:580), nothing launched
    sample, x0 = nan.clone(), nan.clone()
    assert _raw(lib, d, 2, 25, 0.5, x, mo_d, None, sample, x0) == INVALID and b"deterministic" in lib.latte_last_error()
    assert bool(torch.isnan(sample).all()) and bool(torch.isnan(x0).all())
    assert _raw(lib, d, 3, 25, 0.0, x, mo_d, None, sample, x0) == INVALID and b"bad method" in lib.latte_last_error()
    assert _raw(lib, d, 2, 50, 0.0, x, mo_d, None, sample, x0) == INVALID and b"index" in lib.latte_last_error()
    with pytest.raises(AssertionError, match="deterministic"):
        d.ddim_reverse_sample(lambda xx, tt, **k: mo_d, x, _t(d, 25, 3), eta=0.5)
    from latte_amd import LatteError
    with pytest.raises(LatteError, match="one timestep"):
        d.ddim_reverse_sample(lambda xx, tt, **k: mo_d, x, torch.tensor([3, 4, 5]).cuda())


@pytest.mark.parametrize("tag", ["eps_learned", "eps_fixed_large", "xstart_learned"])
def test_forward_methods_are_unchanged_by_the_reverse_method(lib, tag):
    """Methods 0 and 1 beside method 2 on one schedule: they still compute p_sample / ddim_sample (the oracle, at the kernels' bound),
    equal inputs give equal bits, and for eta = 0 the noise pointer plays no part."""
    for index in (0, 25, 49):
        d, s, x_t, mo, nz = _case(tag, index=index)
        x, mo_d, nz_d = x_t.cuda(), mo.cuda(), nz.cuda()
        outs = []
        for method, eta, want in ((0, 0.0, do.p_sample(s, mo, x_t, index, nz, True)),
                                  (1, 0.4, do.ddim_sample(s, mo, x_t, index, nz, 0.4, True)),
                                  (1, 0.0, do.ddim_sample(s, mo, x_t, index, None, 0.0, True))):
            a_s, a_0, b_s, b_0 = (torch.empty_like(x) for _ in range(4))
            assert _raw(lib, d, method, index, eta, x, mo_d, nz_d, a_s, a_0) == 0, lib.latte_last_error()
            assert _raw(lib, d, method, index, eta, x, mo_d, nz_d, b_s, b_0) == 0
            assert torch.equal(a_s, b_s) and torch.equal(a_0, b_0)
            assert rel_l2(a_s, want["sample"]) < TOL and rel_l2(a_0, want["pred_xstart"]) < TOL, (tag, index, method, eta)
            outs.append(a_s)
        r_s, r_0 = torch.empty_like(x), torch.empty_like(x)
        assert _raw(lib, d, 2, index, 0.0, x, mo_d, None, r_s, r_0) == 0
        assert not torch.equal(r_s, outs[2])                                  # up, not down


@pytest.mark.parametrize("tag", sorted(ir.K_TYPES))
def test_consistent_model_walks_the_levels(tag):
    """A model whose output is consistent with (x0*, e*): from q_sample(x0*, 0, e*), step i lands on q_sample(x0*, i + 1, e*) and the
    chain ends at e* itself.  The reference's fp32 arithmetic alone reaches 2.3e-6 (eps types) / 4.0e-6 (x_start types) on "50"; on ""
    the accumulation alone is 9.4e-5, so "50" only.  Then the exact inverse: reverse steps 0 ... T-2, ddim_sample steps T-1 ... 1."""
    import latte_amd
    kw = ir.K_TYPES[tag]
    d, s = latte_amd.create_diffusion("50", **kw), do.Schedule("50", **kw)
    T = s.num_timesteps
    learned = s.var_type == "learned_range"
    x0, e = ir.kernel_x_start(ir.K_SHAPES[0])
    levels = [ir.q_level(s, x0, e, lv).cuda() for lv in range(T + 1)]
    x0d = x0.cuda()
    for clip in (False, True):
        x, worst, worst_x0 = levels[0].clone(), 0.0, 0.0
        for i in range(T):
            r = _reverse(d, ir.consistent_model_out(s, x, i, x0d, learned), x, i, clip)
            x = r["sample"]
            err = rel_l2(x, levels[i + 1])
            worst, worst_x0 = max(worst, err), max(worst_x0, rel_l2(r["pred_xstart"], x0))     # x_0: amplified by sqrt_recip, recorded only
            assert err < TOL, (tag, clip, i, err)
            if i == T - 2:
                top = x.clone()
        assert rel_l2(x, e) < TOL
        ir.record(f"consistent::{tag}::clip{int(clip)}", {"level": worst, "pred_xstart": worst_x0})
        x = top                                                               # level T-1: where ddim_sample_loop starts
        for i in range(T - 1, 0, -1):
            mo = ir.consistent_model_out(s, x, i, x0d, learned)
            x = d.ddim_sample(lambda xx, tt, **k: mo, x, _t(d, i, x.shape[0]), clip_denoised=clip, model_kwargs={})["sample"]
        back = rel_l2(x, levels[0])
        print(tag, clip, "worst level error", worst, "round trip", back)
        ir.record(f"consistent::{tag}::clip{int(clip)}::round_trip", back)
        assert back < TOL, (tag, clip, back)
