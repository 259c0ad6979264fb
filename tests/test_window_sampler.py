"""Sampling clips longer than ``num_frames`` with overlapping temporal windows, end to end on fixture M (tests/bpd_reference.py: a
two-block class-conditional Latte, gates N(0, 0.1), B = 2, F = 4, 8 x 8 latents), f16 operands, ``max_batch`` 12 (the guided cases run
4 x 2 = 8 clips, ddpm10_L8_s1 2 x 5 = 10): ``latte_sample_loop_windows`` / ``latte_sample_plan_loop_windows`` as ONE engine call
against the fp32 restatement of tests/window_reference.py, the public ``SpacedDiffusion.window_sample_loop`` on its fused and its
step-by-step path, and the properties the scheme has by construction, bit for bit.

Bound: the project's 1e-3 parity bar (relative L2) on the final sample and on the trail at the executed indices CHECKPOINTS of
tests/known_reference.py (0, 24, 48, 49 of "50"; 0, 4, 8, 9 of "10" -- for Heun's 19 evaluations these are evaluations, and the last
one is compared as well).  Choice of cases: a perturbation of every model output by 3e-4 of its rms (independent N(0, 1) per element,
i.e. 3e-4 relative L2 -- the shape of operand rounding) moves the restated chains' final samples by
    ddim_L10_s3 3.67e-4   ddpm_L9_s3_tail 1.30e-4   ddim_eta1_L7_s2_clip0 8.44e-5   guided_L6_s2 3.30e-4   ddpm10_L8_s1 2.53e-4
    dpm10_L7_s2 1.23e-4 (dpmsolver++, "10", L 7, stride 2: starts 0, 2, 3)   heun10_L6_s2 1.16e-4 (heun, "10", guided, L 6, stride 2)
on the CPU (``PYTHONPATH=. python tests/window_reference.py`` prints them): every one below half the bar, so all seven are kept.

Fused against step by step: TOL_PATHS = 1e-4, as tests/test_known_sampler.py.

The refusal of H * W % 4 != 0 cannot be reached through a chain here (an even ``input_size`` always has H * W % 4 == 0); it is the
``window_check`` the chains share with ``latte_window_gather`` / ``latte_window_merge``, where tests/test_window_kernels.py provokes it."""
import numpy as np
import pytest
import torch

import window_reference as wr
from _util import engine_model, rel_l2

pytestmark = pytest.mark.gpu
TOL = 1e-3
TOL_PATHS = 1e-4
INVALID, STATE = 1, 3
METHOD = {"ddpm": 0, "ddim": 1}
MAX_BATCH = 12
_CACHE = {}


def _fixture(name):
    """-> (case dict with GPU tensors under "gpu", diffusion, model); one engine for the module."""
    import latte_amd
    if "model" not in _CACHE:
        c = wr.case_inputs("ddim_L10_s3")
        _CACHE["model"] = engine_model(c["kw"], c["sd"], "f16", max_batch=MAX_BATCH)
    if name not in _CACHE:
        c = wr.case_inputs(name)
        c["gpu"] = {k: c[k].cuda().contiguous() for k in ("x_T", "noise", "y")}
        c["d"] = latte_amd.create_diffusion(c["spec"])
        c["linear"] = c["method"] in wr.LINEAR
        if c["linear"]:
            sch = c["d"].linear_scheduler(c["method"])
            c["plan"] = np.ascontiguousarray(sch.engine_plan(), dtype=np.float64)
            c["sigma0"] = float(sch.init_noise_sigma)
        _CACHE[name] = c
    c = _CACHE[name]
    return c, c["d"], _CACHE["model"]


def _nan(n, x):
    return torch.full((n,) + tuple(x.shape), float("nan"), device="cuda")


def _raw(lib, c, d, m, x=None, y="y", noise="noise", L=None, stride=None, batch=None, guided=None, start=None, end=0, windows=True):
    """latte_sample_loop_windows (windows=False: latte_sample_loop_ex) on a copy of x -> (rc, x after, trail_sample, trail_x0), NaN where
    nothing was written."""
    from latte_amd._lib import ptr, stream_ptr
    g = c["gpu"]
    xx = (g["x_T"] if x is None else x).clone()
    pick = lambda v: g[v] if isinstance(v, str) else v
    guided = int(c["guided"]) if guided is None else guided
    T = d.num_timesteps
    start = T - 1 if start is None else start
    B = xx.shape[0] if batch is None else batch
    ts, t0 = _nan(max(start - end + 1, 1), xx), _nan(max(start - end + 1, 1), xx)
    args = (m.engine(MAX_BATCH, guided=bool(guided)), d._h, METHOD[c["method"]], c["eta"], int(c["clip"]), guided,
            wr.M_CFG_SCALE if guided else 1.0, ptr(xx), ptr(pick(y)), B, start, end, ptr(pick(noise)), ptr(ts), ptr(t0))
    if windows:
        rc = lib.latte_sample_loop_windows(*args, xx.shape[1] if L is None else L, c["stride"] if stride is None else stride, stream_ptr())
    else:
        rc = lib.latte_sample_loop_ex(*args, stream_ptr())
    torch.cuda.synchronize()
    return rc, xx, ts, t0


def _raw_plan(lib, c, d, m, x=None, y="y", noise=None, L=None, stride=None, batch=None, guided=None, plan=None, windows=True):
    """latte_sample_plan_loop_windows (windows=False: latte_sample_plan_loop) on a copy of x (already scaled by init_noise_sigma) ->
    (rc, x after, trail_sample)."""
    from latte_amd._lib import check, ptr, stream_ptr
    g = c["gpu"]
    xx = (g["x_T"] * c["sigma0"] if x is None else x).clone()
    pick = lambda v: g[v] if isinstance(v, str) else v
    guided = int(c["guided"]) if guided is None else guided
    plan = c["plan"] if plan is None else plan
    B = xx.shape[0] if batch is None else batch
    ts = _nan(plan.shape[0], xx)
    eng = m.engine(MAX_BATCH, guided=bool(guided))
    check(lib.latte_engine_set_option(eng, b"train_timesteps", d.original_num_steps))
    args = (eng, guided, wr.M_CFG_SCALE if guided else 1.0, ptr(xx), ptr(pick(y)), B, plan.shape[0], plan.ctypes.data, ptr(pick(noise)), ptr(ts))
    if windows:
        rc = lib.latte_sample_plan_loop_windows(*args, xx.shape[1] if L is None else L, c["stride"] if stride is None else stride, stream_ptr())
    else:
        rc = lib.latte_sample_plan_loop(*args, stream_ptr())
    torch.cuda.synchronize()
    return rc, xx, ts


def _fused(lib, name):
    """The case as ONE engine call -> (x after, trail_sample, trail_x0 or None)."""
    key = ("fused", name)
    if key not in _CACHE:
        c, d, m = _fixture(name)
        if c["linear"]:
            rc, xx, ts = _raw_plan(lib, c, d, m)
            t0 = None
        else:
            rc, xx, ts, t0 = _raw(lib, c, d, m)
        assert rc == 0, lib.latte_last_error()
        _CACHE[key] = (xx, ts, t0)
    return _CACHE[key]


@pytest.mark.parametrize("name", list(wr.CASES))
def test_fused_chain_matches_the_restatement(lib, name):
    import latte_amd
    c, d, m = _fixture(name)
    assert latte_amd.window_starts(c["L"], c["F"], c["stride"]) == wr.STARTS[name]
    xx, ts, t0 = _fused(lib, name)
    want = wr.restatement(name)
    assert want.shape == ts.shape
    keep = sorted(set(wr.CHECKPOINTS[c["spec"]]) | {ts.shape[0] - 1})
    err = {k: rel_l2(ts[k], want[k]) for k in keep}
    print(name, "relative L2 at executed indices", err)
    assert torch.isfinite(ts).all() and torch.equal(xx, ts[-1])
    assert all(v < TOL for v in err.values()), err
    if c["guided"]:            # the halves of the doubled batch stay bit-identical
        assert torch.equal(ts[:, :2], ts[:, 2:])
    if t0 is not None:
        assert torch.isfinite(t0).all()
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


@pytest.mark.parametrize("name", ["ddim_L10_s3", "ddim_eta1_L7_s2_clip0", "guided_L6_s2", "ddpm10_L8_s1", "dpm10_L7_s2", "heun10_L6_s2"])
def test_public_loop_fused_is_one_call_and_matches_the_step_by_step_path(monkeypatch, lib, name):
    names = ["latte_sample_loop_windows", "latte_sample_plan_loop_windows", "latte_sample_loop_ex", "latte_sample_plan_loop", "latte_forward",
             "latte_forward_with_cfg", "latte_sampler_step_ex", "latte_window_gather", "latte_window_merge"]
    calls = _count(monkeypatch, lib, names)
    c, d, m = _fixture(name)
    g = c["gpu"]
    xx, ts, t0 = _fused(lib, name)
    for k in calls:
        calls[k] = 0
    fn = m.forward_with_cfg if c["guided"] else m.forward
    mk = dict(y=g["y"], cfg_scale=wr.M_CFG_SCALE) if c["guided"] else dict(y=g["y"])
    kw = dict(noise=g["x_T"], method=c["method"], stride=c["stride"], clip_denoised=c["clip"], model_kwargs=mk, eta=c["eta"])
    if not c["linear"]:
        kw["step_noise"] = g["noise"]
    x_before = g["x_T"].clone()
    out = d.window_sample_loop(fn, g["x_T"].shape, **kw)
    one = "latte_sample_plan_loop_windows" if c["linear"] else "latte_sample_loop_windows"
    assert calls == dict.fromkeys(names, 0) | {one: 1}, calls                              # one segment: ONE engine call
    assert torch.equal(out, xx) and torch.equal(g["x_T"], x_before)                        # the raw call's bits; the input is not written
    for k in calls:
        calls[k] = 0
    stepped = list(d.window_sample_loop_progressive(lambda x_, t_, **k_: fn(x_, t_, **k_), g["x_T"].shape, num_frames=c["F"], **kw))
    n = ts.shape[0]
    fwd = "latte_forward_with_cfg" if c["guided"] else "latte_forward"
    want_calls = {fwd: n, "latte_window_gather": n, "latte_window_merge": n} | ({} if c["linear"] else {"latte_sampler_step_ex": n})
    assert calls == dict.fromkeys(names, 0) | want_calls, calls
    assert len(stepped) == n
    paths = max(rel_l2(stepped[k]["sample"], ts[k]) for k in range(n))
    print(name, "fused vs step by step, worst index", paths)
    assert paths < TOL_PATHS, paths
    # the progressive generator on the engine path hands out the raw call's trails
    trail = list(d.window_sample_loop_progressive(fn, g["x_T"].shape, **kw))
    assert len(trail) == n and all(torch.equal(trail[k]["sample"], ts[k]) for k in range(n))
    if t0 is not None:
        assert all(torch.equal(trail[k]["pred_xstart"], t0[k]) for k in range(n))


def test_a_callable_bound_to_a_plain_object_gets_its_kwargs_repeated_per_window(lib):
    """The step-by-step path on something that is no latte_amd.Latte method: the clips, per-window timesteps and labels it is called with."""
    c, d, m = _fixture("ddpm10_L8_s1")
    g = c["gpu"]
    seen = []

    class Plain:
        num_frames = 4

        def __call__(self, x, t, y=None, flag=None):
            seen.append((tuple(x.shape), t.tolist(), y.tolist(), flag))
            return m.forward(x, t, y=y)

    xx, ts, t0 = _fused(lib, "ddpm10_L8_s1")
    out = d.window_sample_loop(Plain(), g["x_T"].shape, noise=g["x_T"], method="ddpm", stride=1, model_kwargs=dict(y=g["y"], flag="kept"),
                               step_noise=g["noise"])
    assert len(seen) == 10 and seen[0] == ((10, 4, 4, 8, 8), [d.timestep_map[-1]] * 10, [1] * 5 + [3] * 5, "kept")
    assert rel_l2(out, xx) < TOL_PATHS


# ---------------------------------------------------------------------------- bit for bit against the plain loops
def _further_step(lib, c, d, m, x, y, guided):
    """One further engine-drawn DDPM step on x through the plain loop: the Philox offset the chain left behind."""
    cc = dict(c, method="ddpm", eta=0.0, clip=True)
    rc, xx, _, _ = _raw(lib, cc, d, m, x=x, y=y, noise=None, guided=guided, start=5, end=5, windows=False)
    assert rc == 0, lib.latte_last_error()
    return xx


@pytest.mark.parametrize("drawn", [False, True])
@pytest.mark.parametrize("stride", [1, 3, 4])
def test_total_frames_equal_to_num_frames_is_the_plain_sample_loop(lib, stride, drawn):
    c, d, m = _fixture("ddpm_L9_s3_tail")
    g = c["gpu"]
    x = g["x_T"][:, :4].contiguous()
    nz = None if drawn else g["noise"][:, :, :4].contiguous()
    got = {}
    for win in (True, False):
        m.set_engine_option("seed", 91, batch=MAX_BATCH)
        rc, xx, ts, t0 = _raw(lib, c, d, m, x=x, noise=nz, stride=stride, windows=win)
        assert rc == 0, lib.latte_last_error()
        got[win] = (xx, ts, t0, _further_step(lib, c, d, m, xx, g["y"], 0))
    assert all(torch.equal(a, b) for a, b in zip(got[True], got[False]))
    assert torch.isfinite(got[True][1]).all() and not torch.equal(got[True][0], got[True][3])


@pytest.mark.parametrize("method,drawn", [("euler_a", False), ("euler_a", True), ("dpmsolver++", False), ("heun", False)])
def test_total_frames_equal_to_num_frames_is_the_plain_plan_loop(lib, method, drawn):
    c, d, m = _fixture("dpm10_L7_s2")
    g = c["gpu"]
    sch = d.linear_scheduler(method)
    plan = np.ascontiguousarray(sch.engine_plan(), dtype=np.float64)
    x = (g["x_T"][:, :4] * float(sch.init_noise_sigma)).contiguous()
    nz = None
    if method == "euler_a" and not drawn:
        nz = torch.randn((plan.shape[0],) + tuple(x.shape), generator=torch.Generator().manual_seed(3)).cuda()
    got = {}
    for win in (True, False):
        m.set_engine_option("seed", 92, batch=MAX_BATCH)
        rc, xx, ts = _raw_plan(lib, c, d, m, x=x, noise=nz, stride=2, plan=plan, windows=win)
        assert rc == 0, lib.latte_last_error()
        got[win] = (xx, ts, _further_step(lib, c, d, m, xx, g["y"], 0))
    assert all(torch.equal(a, b) for a, b in zip(got[True], got[False])) and torch.isfinite(got[True][1]).all()


@pytest.mark.parametrize("guided", [0, 1])
@pytest.mark.parametrize("drawn", [False, True])
def test_abutting_windows_are_the_plain_loop_on_the_stacked_clips(lib, guided, drawn):
    """L = 2 F at stride F: two windows that do not overlap -- the chain is the plain loop on the 2 N clips, labels and noise stacked
    the same way (clip g * 2 + w: the contiguous reshape of [N, 2 F, ...] to [2 N, F, ...])."""
    c, d, m = _fixture("guided_L6_s2" if guided else "ddpm_L9_s3_tail")
    g = c["gpu"]
    z = torch.randn((2, 8) + tuple(g["x_T"].shape[2:]), generator=torch.Generator().manual_seed(7)).cuda()
    nz = torch.randn((d.num_timesteps, 2, 8) + tuple(z.shape[2:]), generator=torch.Generator().manual_seed(8)).cuda()
    if guided:
        z, nz = torch.cat([z, z]).contiguous(), torch.cat([nz, nz], dim=1).contiguous()
    G = z.shape[0]
    stack = lambda t: t.reshape(t.shape[:-5] + (2 * G, 4) + tuple(t.shape[-3:]))
    cc = dict(c, method="ddpm", eta=0.0)
    got = {}
    for win in (True, False):
        m.set_engine_option("seed", 93, batch=MAX_BATCH, guided=bool(guided))
        if win:
            rc, xx, ts, t0 = _raw(lib, cc, d, m, x=z, noise=None if drawn else nz, stride=4)
            xx, ts, t0 = stack(xx), stack(ts), stack(t0)
        else:
            rc, xx, ts, t0 = _raw(lib, cc, d, m, x=stack(z), y=g["y"].repeat_interleave(2).contiguous(), noise=None if drawn else stack(nz),
                                  windows=False)
        assert rc == 0, lib.latte_last_error()
        y2 = g["y"].repeat_interleave(2).contiguous()
        got[win] = (xx, ts, t0, _further_step(lib, cc, d, m, xx, y2, guided))
    assert all(torch.equal(a, b) for a, b in zip(got[True], got[False])) and torch.isfinite(got[True][1]).all()


def test_segments_of_the_public_loop_compose_bit_for_bit(monkeypatch, lib):
    c, d, m = _fixture("ddpm10_L8_s1")
    g = c["gpu"]
    xx, ts, t0 = _fused(lib, "ddpm10_L8_s1")
    calls = _count(monkeypatch, lib, ["latte_sample_loop_windows"])
    monkeypatch.setattr(type(d), "SEGMENT_BYTES", 4 * g["x_T"].numel() * 4)
    out = d.window_sample_loop(m.forward, g["x_T"].shape, noise=g["x_T"], method="ddpm", stride=1, model_kwargs=dict(y=g["y"]),
                               step_noise=g["noise"])
    assert calls == {"latte_sample_loop_windows": 3} and torch.equal(out, xx)             # 4 + 4 + 2 indices


# ---------------------------------------------------------------------------- refusals
def _untouched(xx, x, *trails):
    return torch.equal(xx, x) and all(bool(torch.isnan(t).all()) for t in trails)


def test_refusals_leave_x_untouched(lib):
    import latte_amd
    c, d, m = _fixture("ddpm_L9_s3_tail")
    g = c["gpu"]
    x, T = g["x_T"], d.num_timesteps
    assert m.max_batch == MAX_BATCH
    big = torch.cat([x, x, x]).contiguous()                                   # 6 rows x 3 windows = 18 clips > 12
    for kw, code, text in ((dict(L=3), INVALID, b"total_frames"), (dict(stride=0), INVALID, b"stride"), (dict(stride=-1), INVALID, b"stride"),
                           (dict(stride=5), INVALID, b"stride"), (dict(start=T), INVALID, b"index range"), (dict(y=None), INVALID, b"needs y"),
                           (dict(batch=MAX_BATCH + 1), STATE, b"max_batch"),
                           (dict(x=big, y=torch.cat([g["y"]] * 3).contiguous()), STATE, b"clips")):
        rc, xx, ts, t0 = _raw(lib, c, d, m, **kw)
        x_in = kw.get("x", x)
        assert rc == code and text in lib.latte_last_error() and b"sample_loop_windows" in lib.latte_last_error(), (kw, lib.latte_last_error())
        assert _untouched(xx, x_in, ts, t0), kw
    # the shared checks come first, in their order: an odd guided batch before the window set
    x3 = torch.cat([x, x[:1]]).contiguous()
    rc, xx, ts, t0 = _raw(lib, c, d, m, x=x3, y=torch.cat([g["y"], g["y"][:1]]).contiguous(), guided=1, stride=0)
    assert rc == INVALID and b"doubled batch" in lib.latte_last_error() and _untouched(xx, x3, ts, t0)
    rc, xx, ts, t0 = _raw(lib, c, latte_amd.create_diffusion("50", learn_sigma=False), m, stride=0)
    assert rc == INVALID and b"learn_sigma" in lib.latte_last_error() and _untouched(xx, x, ts, t0)
    # the plan loop
    cp, dp, _ = _fixture("dpm10_L7_s2")
    xp = cp["gpu"]["x_T"]
    for kw, code, text in ((dict(L=3), INVALID, b"total_frames"), (dict(stride=0), INVALID, b"stride"), (dict(stride=5), INVALID, b"stride"),
                           (dict(stride=1, x=torch.cat([xp] * 4).contiguous(), y=torch.cat([cp["gpu"]["y"]] * 4).contiguous()), STATE, b"clips"),
                           (dict(y=None), INVALID, b"needs y")):
        rc, xx, ts = _raw_plan(lib, cp, dp, m, **kw)
        x_in = kw.get("x", xp * cp["sigma0"])
        assert rc == code and text in lib.latte_last_error() and b"sample_plan_loop_windows" in lib.latte_last_error(), (kw, lib.latte_last_error())
        assert _untouched(xx, x_in, ts), kw
    bad = cp["plan"].copy()
    bad[0, 0] = 0.5                                                           # the plan's own checks come before the window set
    rc, xx, ts = _raw_plan(lib, cp, dp, m, plan=bad, stride=0)
    assert rc == INVALID and b"timestep" in lib.latte_last_error() and _untouched(xx, xp * cp["sigma0"], ts)
