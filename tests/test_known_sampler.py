"""Known-region sampling end to end on fixture M (tests/bpd_reference.py: a two-block class-conditional Latte, gates N(0, 0.1), B = 2,
F = 4, 8 x 8 latents), f16 operands: ``latte_sample_loop_known`` as ONE engine call against the fp32 restatement of
tests/known_reference.py, the public ``SpacedDiffusion.known_sample_loop`` on its fused and its step-by-step path, and the properties
the scheme has by construction, bit for bit.

Bound: the project's 1e-3 parity bar (relative L2) on the final sample and on three intermediate trail entries (executed indices 0,
24, 48 of "50"; 0, 4, 8 of "10").  Choice of cases: a perturbation of every model output by 3e-4 of its rms (independent N(0, 1) per
element, i.e. 3e-4 relative L2 -- the shape of operand rounding, which has no common sign) moves the restated chains' final samples by
    ddim_keyframes 4.2e-4   ddpm_prefix 1.2e-4   ddpm_box_clip0 1.0e-4   ddim_eta1_box 1.5e-4   guided 2.8e-4   ddpm_10x3 3.0e-4
on the CPU (``PYTHONPATH=. python tests/known_reference.py`` prints them): every one below half the bar, so all six are kept, the resampled one at
``resample = 3``.  A common scale error of 3e-4 (every output times 1 + 3e-4) is amplified more by the deterministic chains: 8.5e-4
(ddim_keyframes), 5.3e-4 (guided), 8.3e-4 at index 1 of ddpm_10x3; 1.9 - 2.7e-4 for the others.

Fused against step by step: TOL_PATHS = 1e-4, as tests/test_invert_loop.py."""
import pytest
import torch

import known_reference as kr
from _util import engine_model, rel_l2

pytestmark = pytest.mark.gpu
TOL = 1e-3
TOL_PATHS = 1e-4
INVALID, STATE = 1, 3
METHOD = {"ddpm": 0, "ddim": 1}
_CACHE = {}


def _fixture(name):
    """-> (case dict with GPU tensors under "gpu", diffusion, model); one engine for the module."""
    import latte_amd
    if "model" not in _CACHE:
        c = kr.case_inputs("ddim_keyframes")
        _CACHE["model"] = engine_model(c["kw"], c["sd"], "f16", max_batch=4)
    if name not in _CACHE:
        c = kr.case_inputs(name)
        c["gpu"] = {k: c[k].cuda().contiguous() for k in ("x_T", "known", "mask", "slabs", "y")}
        c["d"] = latte_amd.create_diffusion(c["spec"])
        _CACHE[name] = c
    c = _CACHE[name]
    return c, c["d"], _CACHE["model"]


def _raw(lib, c, d, m, start=None, end=0, resample=None, blend_start=1, noise="slabs", x=None, known="known", mask="mask", batch=None,
         method=None, guided=None, y="y", trails=True):
    """latte_sample_loop_known on a copy of x -> (rc, x after, trail_sample, trail_x0), NaN where nothing was written."""
    from latte_amd._lib import ptr, stream_ptr
    g = c["gpu"]
    T = d.num_timesteps
    start = T - 1 if start is None else start
    xx = (g["x_T"] if x is None else x).clone()
    B = xx.shape[0] if batch is None else batch
    pick = lambda v: g[v] if isinstance(v, str) else v
    guided = int(c["guided"]) if guided is None else guided
    n = max(start - end + 1, 1)
    ts, t0 = (torch.full((n,) + tuple(xx.shape), float("nan"), device="cuda") for _ in range(2)) if trails else (None, None)
    rc = lib.latte_sample_loop_known(m.engine(xx.shape[0], guided=bool(guided)), d._h, METHOD[c["method"]] if method is None else method,
                                     c["eta"], int(c["clip"]), guided, kr.M_CFG_SCALE if guided else 1.0, ptr(xx), ptr(pick(y)), B, start, end,
                                     ptr(pick(known)), ptr(pick(mask)), c["resample"] if resample is None else resample, blend_start,
                                     ptr(pick(noise)), ptr(ts), ptr(t0), stream_ptr())
    torch.cuda.synchronize()
    return rc, xx, ts, t0


def _fused(lib, name):
    key = ("fused", name)
    if key not in _CACHE:
        c, d, m = _fixture(name)
        rc, xx, ts, t0 = _raw(lib, c, d, m)
        assert rc == 0, lib.latte_last_error()
        _CACHE[key] = (xx, ts, t0)
    return _CACHE[key]


@pytest.mark.parametrize("name", list(kr.CASES))
def test_fused_chain_matches_the_restatement(lib, name):
    c, d, m = _fixture(name)
    xx, ts, t0 = _fused(lib, name)
    want = kr.restatement(name)
    keep = kr.CHECKPOINTS[c["spec"]]
    err = {k: rel_l2(ts[k], want[j]) for j, k in enumerate(keep)}
    print(name, "relative L2 at executed indices", err)
    assert torch.isfinite(ts).all() and torch.isfinite(t0).all() and torch.equal(xx, ts[-1])
    assert all(v < TOL for v in err.values()), err
    # the known part of the result is the known clip, bit for bit; the rest is not
    m5 = c["gpu"]["mask"][:, :, None].expand_as(xx)
    assert torch.equal(xx[m5 == 1], c["gpu"]["known"][m5 == 1]) and not torch.equal(xx[m5 == 0], c["gpu"]["known"][m5 == 0])
    if c["guided"]:            # the halves of the doubled batch stay bit-identical
        assert torch.equal(ts[:, :2], ts[:, 2:])
    if c["clip"]:
        assert float(t0.abs().max()) <= 1.0


def _count(monkeypatch, lib, names):
    calls = {n: 0 for n in names}
    for n in names:
        real = getattr(lib, n)

        def wrapper(*a, _real=real, _n=n):
            calls[_n] += 1
            return _real(*a)
        monkeypatch.setattr(lib, n, wrapper, raising=False)
    return calls


@pytest.mark.parametrize("name", ["ddim_keyframes", "ddim_eta1_box", "guided", "ddpm_10x3"])
def test_public_loop_fused_is_one_call_and_matches_the_step_by_step_path(monkeypatch, lib, name):
    names = ["latte_sample_loop_known", "latte_sample_loop_ex", "latte_forward", "latte_forward_with_cfg", "latte_sampler_step_ex", "latte_known_blend"]
    calls = _count(monkeypatch, lib, names)
    c, d, m = _fixture(name)
    g = c["gpu"]
    xx, ts, t0 = _fused(lib, name)
    for k in calls:
        calls[k] = 0
    fn = m.forward_with_cfg if c["guided"] else m.forward
    mk = dict(y=g["y"], cfg_scale=kr.M_CFG_SCALE) if c["guided"] else dict(y=g["y"])
    kw = dict(method=c["method"], noise=g["x_T"], clip_denoised=c["clip"], model_kwargs=mk, eta=c["eta"], resample=c["resample"],
              chain_noise=g["slabs"])
    x_before = g["x_T"].clone()
    out = d.known_sample_loop(fn, g["x_T"].shape, g["known"], g["mask"], **kw)
    assert calls == dict.fromkeys(names, 0) | {"latte_sample_loop_known": 1}, calls        # one segment: ONE engine call
    assert torch.equal(out, xx) and torch.equal(g["x_T"], x_before)                        # the raw call's bits; the input is not written
    for k in calls:
        calls[k] = 0
    stepped = list(d.known_sample_loop_progressive(lambda x_, t_, **k_: fn(x_, t_, **k_), g["x_T"].shape, g["known"], g["mask"], **kw))
    T, R = d.num_timesteps, c["resample"]
    fwd = "latte_forward_with_cfg" if c["guided"] else "latte_forward"
    assert calls == dict.fromkeys(names, 0) | {fwd: T * R, "latte_sampler_step_ex": T * R, "latte_known_blend": T * R + 1}, calls
    assert len(stepped) == T
    paths = max(rel_l2(stepped[k]["sample"], ts[k]) for k in range(T))
    print(name, "fused vs step by step, worst index", paths)
    assert paths < TOL_PATHS, paths
    m5 = g["mask"][:, :, None].expand_as(xx)
    assert torch.equal(stepped[-1]["sample"][m5 == 1], g["known"][m5 == 1])
    # the progressive generator on the engine path hands out the raw call's trails
    trail = list(d.known_sample_loop_progressive(fn, g["x_T"].shape, g["known"], g["mask"], **kw))
    assert len(trail) == T and all(torch.equal(trail[k]["sample"], ts[k]) and torch.equal(trail[k]["pred_xstart"], t0[k]) for k in range(T))


def test_segments_of_the_public_loop_compose_bit_for_bit(monkeypatch, lib):
    """SEGMENT_BYTES small enough for a few indices per segment: one engine call per segment, the bits of the single call."""
    c, d, m = _fixture("ddpm_10x3")
    g = c["gpu"]
    xx, ts, t0 = _fused(lib, "ddpm_10x3")
    calls = _count(monkeypatch, lib, ["latte_sample_loop_known"])
    per_index = g["x_T"].numel() * 4 * 3 * c["resample"]
    monkeypatch.setattr(type(d), "SEGMENT_BYTES", 4 * per_index)
    out = d.known_sample_loop(m.forward, g["x_T"].shape, g["known"], g["mask"], method="ddpm", noise=g["x_T"], model_kwargs=dict(y=g["y"]),
                              resample=3, chain_noise=g["slabs"])
    assert calls == {"latte_sample_loop_known": 3} and torch.equal(out, xx)               # 4 + 4 + 2 indices


def test_all_zero_mask_is_the_plain_chain_bit_for_bit(lib):
    from latte_amd._lib import check, ptr, stream_ptr
    c, d, m = _fixture("ddpm_prefix")
    g = c["gpu"]
    T = d.num_timesteps
    rc, xx, ts, t0 = _raw(lib, c, d, m, mask=torch.zeros_like(g["mask"]))
    assert rc == 0, lib.latte_last_error()
    # slab order of DDPM, resample 1: the start blend, then (step, blend) for every index above 0; latte_sample_loop_ex reads row k at step k
    rows = torch.cat([g["slabs"][1:2 * (T - 1):2], torch.zeros_like(g["slabs"][:1])]).contiguous()
    assert rows.shape[0] == T
    plain = g["x_T"].clone()
    ps, p0 = torch.empty_like(ts), torch.empty_like(t0)
    check(lib.latte_sample_loop_ex(m.engine(2), d._h, 0, 0.0, 1, 0, 1.0, ptr(plain), ptr(g["y"]), 2, T - 1, 0, ptr(rows), ptr(ps), ptr(p0), stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(xx, plain) and torch.equal(ts, ps) and torch.equal(t0, p0)


def test_all_one_mask_returns_the_known_clip(lib):
    c, d, m = _fixture("ddim_keyframes")
    g = c["gpu"]
    rc, xx, ts, t0 = _raw(lib, c, d, m, mask=torch.ones_like(g["mask"]))
    assert rc == 0 and torch.equal(xx, g["known"])


@pytest.mark.parametrize("name,k", [("ddpm_prefix", 20), ("ddpm_10x3", 4), ("ddim_eta1_box", 1)])
def test_a_chain_split_into_two_calls_is_the_single_call(lib, name, k):
    c, d, m = _fixture(name)
    g = c["gpu"]
    T = d.num_timesteps
    xx, ts, t0 = _fused(lib, name)
    n1 = d.known_chain_slabs(c["method"], c["eta"], c["resample"], T - 1, k, True)
    n2 = d.known_chain_slabs(c["method"], c["eta"], c["resample"], k - 1, 0, False)
    assert n1 + n2 == g["slabs"].shape[0]
    rc, mid, ts1, _ = _raw(lib, c, d, m, start=T - 1, end=k, noise=g["slabs"][:n1].contiguous())
    assert rc == 0 and torch.equal(mid, ts[T - 1 - k])
    rc, end, ts2, _ = _raw(lib, c, d, m, start=k - 1, end=0, blend_start=0, noise=g["slabs"][n1:].contiguous(), x=mid)
    assert rc == 0 and torch.equal(end, xx) and torch.equal(torch.cat([ts1, ts2]), ts)


@pytest.mark.parametrize("name", ["ddpm_10x3", "ddim_keyframes"])
def test_a_philox_drawn_chain_is_the_chain_fed_the_same_draws(lib, name):
    from latte_amd._lib import check, ptr, stream_ptr
    c, d, m = _fixture(name)
    g = c["gpu"]
    seed = 77
    m.set_engine_option("seed", seed, batch=2)
    rc, drawn, ts, _ = _raw(lib, c, d, m, noise=None)
    assert rc == 0, lib.latte_last_error()
    slabs = torch.empty_like(g["slabs"])
    numel = g["x_T"].numel()
    for j in range(slabs.shape[0]):        # slab j of the chain is the generator's slab at offset j * numel
        check(lib.latte_debug_fill_normal(ptr(slabs[j]), numel, seed, j * numel, stream_ptr()))
    rc, fed, ts2, _ = _raw(lib, c, d, m, noise=slabs)
    assert rc == 0 and torch.equal(drawn, fed) and torch.equal(ts, ts2)
    rc, again, _, _ = _raw(lib, c, d, m, noise=None)                 # the stream has advanced: a second chain draws other noise
    assert rc == 0 and not torch.equal(again, drawn)
    m.set_engine_option("seed", seed, batch=2)
    rc, reset, _, _ = _raw(lib, c, d, m, noise=None)
    assert rc == 0 and torch.equal(reset, drawn)


def test_resample_one_is_the_path_without_repetition(lib):
    """The chain composed by hand from what existed before -- one latte_sample_loop_ex step, then one latte_known_blend -- per index."""
    from latte_amd._lib import check, ptr, stream_ptr
    from latte_amd.known import level_coefs
    c, d, m = _fixture("ddpm_prefix")
    g = c["gpu"]
    T = d.num_timesteps
    xx, ts, t0 = _fused(lib, "ddpm_prefix")
    x = g["x_T"].clone()
    B, F, C, H, W = x.shape
    it = iter(g["slabs"])

    def blend(abar, z):
        a, b = level_coefs(abar) if z is not None else (1.0, 0.0)
        check(lib.latte_known_blend(ptr(x), ptr(g["known"]), ptr(g["mask"]), ptr(z), 0, 0, a, b, B, F, C, H * W, 0, stream_ptr()))

    blend(d.alphas_cumprod[T - 1], next(it))
    for i in range(T - 1, -1, -1):
        nz = next(it).contiguous() if i > 0 else None
        check(lib.latte_sample_loop_ex(m.engine(2), d._h, 0, 0.0, 1, 0, 1.0, ptr(x), ptr(g["y"]), 2, i, i, ptr(nz), None, None, stream_ptr()))
        blend(d.alphas_cumprod_prev[i], next(it) if i > 0 else None)
        torch.cuda.synchronize()
        assert torch.equal(x, ts[T - 1 - i]), i
    assert torch.equal(x, xx)


def _untouched(xx, x, ts, t0):
    return torch.equal(xx, x) and bool(torch.isnan(ts).all()) and bool(torch.isnan(t0).all())


def test_refusals_leave_x_untouched(lib):
    import latte_amd
    from latte_amd import LatteError
    c, d, m = _fixture("ddpm_prefix")
    g = c["gpu"]
    x, T = g["x_T"], d.num_timesteps
    for kw, code, text in ((dict(resample=0), INVALID, b"resample"), (dict(resample=-2), INVALID, b"resample"),
                           (dict(known=None), INVALID, b"known and mask"), (dict(mask=None), INVALID, b"known and mask"),
                           (dict(start=T), INVALID, b"index range"), (dict(start=3, end=4), INVALID, b"index range"),
                           (dict(end=-1), INVALID, b"index range"), (dict(method=2), INVALID, b"method"),
                           (dict(batch=m.max_batch + 1), STATE, b"max_batch"), (dict(y=None), INVALID, b"needs y")):
        rc, xx, ts, t0 = _raw(lib, c, d, m, **kw)
        assert rc == code and text in lib.latte_last_error() and _untouched(xx, x, ts, t0), (kw, lib.latte_last_error())
    rc, xx, ts, t0 = _raw(lib, c, latte_amd.create_diffusion("50", learn_sigma=False), m)
    assert rc == INVALID and b"learn_sigma" in lib.latte_last_error() and _untouched(xx, x, ts, t0)
    x3 = torch.cat([x, x[:1]]).contiguous()
    rc, xx, ts, t0 = _raw(lib, c, d, m, x=x3, y=torch.cat([g["y"], g["y"][:1]]).contiguous(), guided=1)
    assert rc == INVALID and b"doubled batch" in lib.latte_last_error() and _untouched(xx, x3, ts, t0)
    # the host interface
    kw = dict(noise=x, model_kwargs=dict(y=g["y"]))
    with pytest.raises(LatteError, match="known must be"):
        d.known_sample_loop(m.forward, x.shape, g["known"][:, :2], g["mask"], **kw)
    with pytest.raises(LatteError, match="known_mask must be"):
        d.known_sample_loop(m.forward, x.shape, g["known"], g["mask"][:, :2], **kw)
    with pytest.raises(LatteError, match="chain_noise must be"):
        d.known_sample_loop(m.forward, x.shape, g["known"], g["mask"], method="ddpm", chain_noise=g["slabs"][:5], **kw)
    with pytest.raises(LatteError, match="linear samplers"):
        d.linear_sample_loop(m.forward, x.shape, known=g["known"], known_mask=g["mask"], **kw)
