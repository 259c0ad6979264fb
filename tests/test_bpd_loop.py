"""Likelihood evaluation end to end: ``SpacedDiffusion.calc_bpd_loop`` (gaussian_diffusion.py:813-866) as ONE latte_bpd_loop call
inside the engine and as the step-by-step loop over a plain model callable, against tests/golden/bpd.npz -- the reference's own
calc_bpd_loop on fixture M of tests/bpd_reference.py (a two-block class-conditional Latte, gates N(0, 0.1), B = 2,
create_diffusion("50")) with the same noise.

Bounds: f16 operands hold the project's 1e-3 parity bar on EVERY entry of vb / xstart_mse / mse / total_bpd (the f16 operand error
alone is about 1.2e-4 on this fixture); prior_bpd involves no model and holds the kernels' 2e-5.  bf16 operands are measured and
recorded, and asserted at the bound tests/test_gpu_parity.py uses for bf16 at this gate scale."""
import os

import numpy as np
import pytest
import torch

import bpd_reference as br
from _util import GOLDEN, engine_model

pytestmark = pytest.mark.gpu
TOL = 1e-3          # the project's parity bar
TOL_PRIOR = 2e-5    # tests/test_bpd_kernels.py
TOL_BF16 = 1e-2     # tests/test_gpu_parity.py: BF16_TOL_AT_TRAINED_GATES
TOL_PATHS = 1e-4    # fused loop against the step-by-step loop: an order under the parity bar
T = 50
_CACHE = {}


def _golden():
    return np.load(os.path.join(GOLDEN, "bpd.npz"))


def _fixture(extras=2, learn_sigma=True, cd="f16"):
    """-> (diffusion, model on the GPU, x0, y, noise) on the device; one engine per variant for the module."""
    import latte_amd
    key = (extras, learn_sigma, cd)
    if key not in _CACHE:
        kw, cfg, sd, x0, y, noise = br.model_inputs(extras, learn_sigma)
        m = engine_model(kw, sd, cd, max_batch=2)
        d = latte_amd.create_diffusion(br.M_SPEC, learn_sigma=learn_sigma)
        _CACHE[key] = (d, m, x0.cuda(), None if y is None else y.cuda(), noise.cuda())
    return _CACHE[key]


def _kwargs(y):
    return {} if y is None else dict(y=y)


def _fused(clip, cd="f16"):
    key = ("fused", clip, cd)
    if key not in _CACHE:
        d, m, x0, y, noise = _fixture(cd=cd)
        r = d.calc_bpd_loop(m.forward, x0, clip, _kwargs(y), noise=noise)
        assert torch.equal(r["total_bpd"], r["vb"].sum(dim=1) + r["prior_bpd"])              # gd:859, exactly (on the device)
        _CACHE[key] = {k: v.cpu() for k, v in r.items()}
    return _CACHE[key]


def _errors(got, want):
    return {k: br.rel_max(got[k].numpy() if torch.is_tensor(got[k]) else got[k], want[k]) for k in br.TABLES}


def _want(clip):
    z = _golden()
    return {k: z[f"M::clip{int(clip)}::{k}"] for k in br.TABLES}


@pytest.mark.parametrize("clip", [True, False], ids=["clip", "noclip"])
def test_fused_loop_matches_reference(clip):
    got = _fused(clip)
    err = _errors(got, _want(clip))
    print("f16", clip, err)
    br.record(f"M::fused::f16::clip{int(clip)}", err)
    assert set(got) == set(br.TABLES) and got["vb"].shape == (2, T)
    assert all(torch.isfinite(v).all() for v in got.values())
    assert all(err[k] < TOL for k in br.TABLES), err
    assert err["prior_bpd"] < TOL_PRIOR, err


@pytest.mark.parametrize("clip", [True, False], ids=["clip", "noclip"])
def test_fused_loop_bf16_operands_recorded(clip):
    err = _errors(_fused(clip, "bf16"), _want(clip))
    print("bf16", clip, err)
    br.record(f"M::fused::bf16::clip{int(clip)}", err)
    assert all(err[k] < TOL_BF16 for k in br.TABLES), err
    assert err["prior_bpd"] < TOL_PRIOR, err


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
    d, m, x0, y, noise = _fixture()
    fused = _fused(True)
    calls = _count(monkeypatch, lib, ["latte_bpd_loop", "latte_forward", "latte_bpd_terms"])
    again = d.calc_bpd_loop(m.forward, x0, True, _kwargs(y), noise=noise)
    assert calls == {"latte_bpd_loop": 1, "latte_forward": 0, "latte_bpd_terms": 0}, calls
    assert all(torch.equal(again[k].cpu(), fused[k]) for k in br.TABLES)                   # and it is reproducible
    for clip in (True, False):
        for k in calls:
            calls[k] = 0
        stepped = d.calc_bpd_loop(lambda xx, tt, **k: m.forward(xx, tt, **k), x0, clip, _kwargs(y), noise=noise)
        assert calls == {"latte_bpd_loop": 0, "latte_forward": T, "latte_bpd_terms": T}, calls
        stepped = {k: v.cpu() for k, v in stepped.items()}
        err = _errors(stepped, _want(clip))
        paths = _errors(stepped, {k: v.numpy() for k, v in _fused(clip).items()})
        print("stepped", clip, err, "fused vs stepped", paths)
        br.record(f"M::stepped::f16::clip{int(clip)}", err)
        br.record(f"M::fused_vs_stepped::f16::clip{int(clip)}", paths)
        assert all(err[k] < TOL for k in br.TABLES) and err["prior_bpd"] < TOL_PRIOR, err
        assert all(paths[k] < TOL_PATHS for k in br.TABLES), paths


def _raw_loop(lib, d, m, x0, y, start, end, noise, batch=None):
    from latte_amd._lib import ptr, stream_ptr
    B = x0.shape[0] if batch is None else batch
    n = start - end + 1
    tabs = tuple(torch.full((B, max(n, 1)), float("nan"), device="cuda") for _ in range(3))
    rc = lib.latte_bpd_loop(m.engine(x0.shape[0]), d._h, 1, ptr(x0), ptr(y), B, start, end, ptr(noise), ptr(tabs[0]), ptr(tabs[1]),
                            ptr(tabs[2]), stream_ptr())
    torch.cuda.synchronize()
    return rc, tuple(t.cpu() for t in tabs)


def test_column_order_and_split_loops(lib):
    d, m, x0, y, noise = _fixture()
    fused = _fused(True)
    full = (fused["vb"], fused["xstart_mse"], fused["mse"])
    # column 0 is t = T-1, column -1 the decoder NLL (index 0): each step run alone with its own noise slice
    rc, last = _raw_loop(lib, d, m, x0, y, T - 1, T - 1, noise[0:1].contiguous())
    assert rc == 0, lib.latte_last_error()
    rc, first = _raw_loop(lib, d, m, x0, y, 0, 0, noise[T - 1:].contiguous())
    assert rc == 0, lib.latte_last_error()
    for j in range(3):
        assert torch.equal(last[j][:, 0], full[j][:, 0]) and torch.equal(first[j][:, 0], full[j][:, T - 1])
    assert not torch.equal(full[0][:, 0], full[0][:, T - 1])
    # 49 ... 25, then 24 ... 0, with the matching noise slices: the same bits as one call
    rc, hi = _raw_loop(lib, d, m, x0, y, T - 1, 25, noise[:25].contiguous())
    assert rc == 0, lib.latte_last_error()
    rc, lo = _raw_loop(lib, d, m, x0, y, 24, 0, noise[25:].contiguous())
    assert rc == 0, lib.latte_last_error()
    for j in range(3):
        assert torch.equal(torch.cat([hi[j], lo[j]], dim=1), full[j])


def test_engine_noise_is_seeded_and_leaves_the_sampler_stream_alone(lib):
    from latte_amd._lib import check, ptr, stream_ptr
    d, m, x0, y, noise = _fixture()
    z = _golden()

    def run(seed):
        m.set_engine_option("seed", seed, batch=2)
        return {k: v.cpu() for k, v in d.calc_bpd_loop(m.forward, x0, False, _kwargs(y)).items()}

    a, b, c = run(5), run(5), run(6)
    assert all(torch.equal(a[k], b[k]) for k in br.TABLES)
    assert not torch.equal(a["mse"], c["mse"])
    # statistical check: the t = T-1 eps-MSE of an untrained model against a unit normal, the golden's value +- 50 %
    want = z["M::clip0::mse"][:, 0]
    for r in (a, c):
        got = r["mse"][:, 0].numpy()
        assert np.all(got > 0.5 * want) and np.all(got < 1.5 * want), (got, want)
        assert all(torch.isfinite(v).all() for v in r.values())

    def sample():     # DDPM steps drawing from the engine's Philox stream (noise = NULL)
        x = x0.clone()
        check(lib.latte_sample_loop(m.engine(2), d._h, 0, 0.0, 1, 1.0, ptr(x), ptr(y), 2, 5, 0, None, None, None, stream_ptr()))
        torch.cuda.synchronize()
        return x.cpu()

    m.set_engine_option("seed", 9, batch=2)
    s1, s2 = sample(), sample()
    assert not torch.equal(s1, s2)                       # the second loop continues the stream
    m.set_engine_option("seed", 9, batch=2)
    t1 = sample()
    d.calc_bpd_loop(m.forward, x0, True, _kwargs(y), noise=noise)      # caller-supplied noise: the Philox offset stays
    t2 = sample()
    assert torch.equal(s1, t1) and torch.equal(s2, t2)


@pytest.mark.parametrize("extras,learn_sigma", [(1, True), (2, False)], ids=["unconditional", "fixed_variance"])
def test_other_models_match_the_restatement(extras, learn_sigma):
    d, m, x0, y, noise = _fixture(extras, learn_sigma)
    want = {k: v.numpy() for k, v in br.model_restatement(extras, learn_sigma, True).items()}
    got = {k: v.cpu() for k, v in d.calc_bpd_loop(m.forward, x0, True, _kwargs(y), noise=noise).items()}
    err = _errors(got, want)
    print(extras, learn_sigma, err)
    br.record(f"M::fused::f16::extras{extras}::learn_sigma{int(learn_sigma)}", err)
    assert all(err[k] < TOL for k in br.TABLES) and err["prior_bpd"] < TOL_PRIOR, err


def test_refusals(lib):
    import latte_amd
    from latte_amd import LatteError
    d, m, x0, y, noise = _fixture()
    with pytest.raises(LatteError, match="learn_sigma"):
        latte_amd.create_diffusion(br.M_SPEC, learn_sigma=False).calc_bpd_loop(m.forward, x0, True, _kwargs(y), noise=noise)
    with pytest.raises(LatteError, match="labels y"):
        d.calc_bpd_loop(m.forward, x0, True, {}, noise=noise)
    rc, tabs = _raw_loop(lib, d, m, x0, None, T - 1, 0, noise)
    assert rc == 1 and b"needs y" in lib.latte_last_error() and all(bool(torch.isnan(t).all()) for t in tabs)
    rc, tabs = _raw_loop(lib, d, m, x0, y, T - 1, 0, noise, batch=m.max_batch + 1)
    assert rc == 3 and b"max_batch" in lib.latte_last_error() and all(bool(torch.isnan(t).all()) for t in tabs)
    for start, end in ((T, 0), (3, 4), (3, -1)):
        rc, tabs = _raw_loop(lib, d, m, x0, y, start, end, noise)
        assert rc == 1 and b"index range" in lib.latte_last_error() and all(bool(torch.isnan(t).all()) for t in tabs)
    x_t = d.q_sample(x0, torch.tensor([3, 3]), noise[0])
    with pytest.raises(LatteError, match="one timestep"):
        d._vb_terms_bpd(m.forward, x0, x_t, torch.tensor([3, 4]).cuda(), True, _kwargs(y))
    out = d._vb_terms_bpd(m.forward, x0, x_t, torch.tensor([3, 3]).cuda(), True, _kwargs(y))
    assert set(out) == {"output", "pred_xstart"} and out["output"].shape == (2,) and out["pred_xstart"].shape == x0.shape
    assert float(out["pred_xstart"].abs().max()) <= 1.0 and torch.isfinite(out["output"]).all()


def test_full_length_chain_properties():
    """create_diffusion("") -- 1000 steps, the chain conditioning in several chunks -- with the engine's own noise."""
    import latte_amd
    _, m, x0, y, _ = _fixture()
    d = latte_amd.create_diffusion("")
    m.set_engine_option("seed", 3, batch=2)
    r = d.calc_bpd_loop(m.forward, x0, True, _kwargs(y))
    assert r["vb"].shape == r["mse"].shape == r["xstart_mse"].shape == (2, 1000)
    assert all(torch.isfinite(v).all() for v in r.values())
    assert torch.equal(r["total_bpd"], r["vb"].sum(dim=1) + r["prior_bpd"])
    assert bool((r["vb"] >= 0).all()) and bool((r["prior_bpd"] > 0).all())
