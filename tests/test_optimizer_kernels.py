"""The optimiser step's kernels (csrc/train.hip: sumsq_kernel, gradnorm_finalize_kernel, adamw_ema_kernel) one launch at a time through
latte_debug_grad_norm and latte_debug_adamw_ema, from GIVEN states -- moments, bias-correction counts, weight decay and loss-scale
counters that the end-to-end tests only ever see at AdamW's step 1.  Every buffer lies inside a larger one whose other elements hold a
sentinel that must come back bit for bit.

AdamW + EMA.  The reference is torch.optim.AdamW's single-tensor rule plus update_ema in fp64 on the same fp32 p, g, m, v, ema, with the
hyper-parameters rounded to fp32 first (they cross the ABI as floats):

    g' = g coef;  p1 = p (1 - lr wd);  m' = b1 m + (1 - b1) g';  v' = b2 v + (1 - b2) g'^2
    denom = sqrt(v') / sqrt(1 - b2^t) + eps;  upd = lr / (1 - b1^t) * m' / denom;  p' = p1 - upd;  ema' = d ema + (1 - d) p'

Bounds, per element, u = 2^-24, counting the kernel's fp32 roundings (it runs without contraction; fp32 divide and square root are
correctly rounded in the library's build):
  m'   g coef (1), 1 - b1 (1), their product (1), m b1 (1), the sum (1): the g term passes 4 roundings, the m term 2
       |dm| <= A_M u (|b1 m| + |(1 - b1) g'|),  A_M = 4
  v'   g'^2 carries 2 x 1 from g' and 1 of its own, 1 - b2 (1), product (1), v b2 (1), sum (1): 6 on the g term, 2 on the v term
       |dv| <= A_V u (|b2 v| + |(1 - b2) g'^2|) = A_V u v',  A_V = 6
  upd  sqrt(v'): A_V / 2 + 1 = 4;  sqrt(1 - b2^t) is formed in fp64 and rounded once (1), the divide (1), + eps (1): denom within 7 u.
       1 - b1^t: b1^t is rounded to fp32 before the subtraction, which loses b1^t / bc1 u against bc1, and the subtraction rounds (1):
       E_BC1 = b1^t / bc1 + 1.  lr / bc1 (1), m' / denom (1), their product (1); m' itself is off by dm, which goes through
       (lr / bc1) / denom -- m' cancels, so this term is taken on  updabs = lr / bc1 * (|b1 m| + |(1 - b1) g'|) / denom >= |upd|, not on |upd|.
       |dupd| <= u (7 + E_BC1 + 3 + A_M) updabs
  p'   lr wd (1, times lr wd: negligible, counted), 1 - lr wd (1), p times it (1), the subtraction (1, on |p'| <= |p| + |upd|)
       |dp| <= u (A_P |p| + B_P updabs),  A_P = 4,  B_P = 15 + E_BC1
  ema' ema d (1), 1 - d (1), p' (1 - d) (1), the sum (1): 3 on the larger count, plus dp through (1 - d)
       |dema| <= u A_E (|d ema| + |(1 - d) p'|) + (1 - d) |dp|,  A_E = 3
The p bound departs from the form |dp| <= u (a |p| + b |upd|) in one respect, named above: b multiplies updabs, because the rounding
of m' does not shrink when its two addends cancel.  None of the constants is fitted.  test_adamw_bounds_on_the_cpu keeps the
bounds honest without a GPU: an fp32 numpy restatement of the kernel, operation for operation, must lie inside them and each of six
plausible mistakes outside -- so the inputs (|g| log-uniform in [1e-9, 1], where eps matters; moments of the gradient's magnitude)
are shown to discriminate.  lr = 3e-3 and ema_decay = 0.99 make the update and the EMA's share of p' large against u |p|.

Gradient norm.  fp64 sum of squares on the GPU against numpy's fp64 sum: only the order differs, so float32(reference) within one
fp32 ulp.  The coefficient is recomputed from the kernel's own norm: min(max_norm / (norm + 1e-6), 1) passes an add and a divide, 2 u
(1e-6 as the fp32 constant the kernel holds, like every hyper-parameter).

Worst err / bound per output is printed by every test; the figures of the MI355X run are in DESIGN.md section 4.7."""
import math

import numpy as np
import pytest
import torch

from test_bookend_kernels import _call, _rc, _sync

gpu = pytest.mark.gpu
U32 = 2.0 ** -24
SENT = -7.25
PAD = 8
LATTE_ERR_INVALID = 1
A_M, A_V, A_P, A_E = 4.0, 6.0, 4.0, 3.0
HYPER = dict(lr=3e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.1, decay=0.99)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda")


def _f32(x):
    return float(np.float32(x))


def _guarded(values, offset=0, dtype=torch.float32):
    """-> (buf, view): `values` copied PAD + offset elements into a buffer that holds SENT everywhere else.  The allocation is 16-byte
    aligned and PAD elements are a multiple of 16 bytes, so offset 0 keeps a float view aligned and offset 1 does not."""
    n = values.numel()
    buf = torch.full((PAD + offset + n + PAD,), SENT, device=values.device, dtype=dtype)
    assert buf.data_ptr() % 16 == 0
    view = buf[PAD + offset:PAD + offset + n]
    view.copy_(values)
    return buf, view


def _guards_intact(tag, buf, view):
    """call after the last read of `view`: it is overwritten."""
    view.fill_(SENT)
    assert bool((buf == SENT).all()), f"{tag}: wrote outside its range"


def _within(tag, got, want, bound):
    err = (got.double() - want).abs()
    bad = ~(err <= bound)
    if bool(bad.any()):
        i = int(torch.nonzero(bad.reshape(-1))[0])
        raise AssertionError(f"{tag}: {int(bad.sum())} of {err.numel()} elements out of bound; first {i}: got {float(got.reshape(-1)[i]):.9e} want "
                             f"{float(want.reshape(-1)[i]):.9e} err {float(err.reshape(-1)[i]):.3e} > {float(bound.reshape(-1)[i]):.3e}; worst err / bound "
                             f"{float((err / bound).max()):.3g}")
    return float((err / bound).max())


# ------------------------------------------------------------------------------------------------ AdamW: reference, bounds, restatement
def adamw_inputs(n, step, g, dev):
    """|g| log-uniform in [1e-9, 1] with random sign; step > 1: m ~ N(0, 1) |g|, v = g^2 10^U(-1, 1), a fresh state otherwise;
    p ~ N(0, 0.05), ema = p + N(0, 1e-3).  All fp32."""
    r = lambda: torch.rand(n, generator=g, device=dev, dtype=torch.float64)
    rn = lambda: torch.randn(n, generator=g, device=dev, dtype=torch.float64)
    gr = 10.0 ** (r() * 9 - 9) * torch.where(r() < 0.5, -1.0, 1.0)
    m = rn() * gr.abs() if step > 1 else torch.zeros_like(gr)
    v = gr * gr * 10.0 ** (r() * 2 - 1) if step > 1 else torch.zeros_like(gr)
    p = rn() * 0.05
    ema = p + rn() * 1e-3
    return tuple(t.float() for t in (p, gr, m, v, ema))


def adamw_ref(p, g, m, v, ema, h, step, coef):
    """-> ({name: fp64 result}, {name: bound}) of one update (module docstring); h: HYPER-like dict, rounded to fp32 here."""
    lr, b1, b2, eps, wd, d = (_f32(h[k]) for k in ("lr", "b1", "b2", "eps", "wd", "decay"))
    p, g, m, v, ema = (t.double() for t in (p, g, m, v, ema))
    gc = g * _f32(coef)
    p1 = p * (1.0 - lr * wd)
    m1 = b1 * m + (1.0 - b1) * gc
    v1 = b2 * v + (1.0 - b2) * gc * gc
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    denom = v1.sqrt() / math.sqrt(bc2) + eps
    p2 = p1 - lr / bc1 * (m1 / denom)
    e2 = d * ema + (1.0 - d) * p2
    mabs = (b1 * m).abs() + ((1.0 - b1) * gc).abs()
    updabs = lr / bc1 * mabs / denom
    e_bc1 = b1 ** step / bc1 + 1.0
    bp = U32 * (A_P * p.abs() + (15.0 + e_bc1) * updabs)
    be = U32 * A_E * ((d * ema).abs() + ((1.0 - d) * p2).abs()) + (1.0 - d) * bp
    return dict(p=p2, m=m1, v=v1, ema=e2), dict(p=bp, m=A_M * U32 * mabs, v=A_V * U32 * v1, ema=be)


MUTANTS = ("eps_in_root", "eps_before_bc", "bc2_unrooted", "bc1_dropped", "ema_old_p", "wd_without_lr")


def adamw_f32(p, g, m, v, ema, h, step, coef, mutant=None):
    """adamw_ema_kernel's `upd` lambda in numpy fp32, one rounding per operation in the kernel's order (numpy arrays in and out)."""
    f = np.float32
    lr, b1, b2, eps, wd, d = (f(h[k]) for k in ("lr", "b1", "b2", "eps", "wd", "decay"))
    one = f(1.0)
    bc1 = one - f(float(b1) ** step)
    bc2_64 = 1.0 - float(b2) ** step
    sqrt_bc2 = f(math.sqrt(bc2_64))
    gi = g * f(coef)
    pi = p * (one - (wd if mutant == "wd_without_lr" else lr * wd))
    mi = m * b1 + gi * (one - b1)
    vi = v * b2 + (gi * gi) * (one - b2)
    if mutant == "eps_in_root":
        denom = np.sqrt(vi + eps) / sqrt_bc2
    elif mutant == "eps_before_bc":
        denom = (np.sqrt(vi) + eps) / sqrt_bc2
    elif mutant == "bc2_unrooted":
        denom = np.sqrt(vi) / f(bc2_64) + eps
    else:
        denom = np.sqrt(vi) / sqrt_bc2 + eps
    pi = pi - (lr if mutant == "bc1_dropped" else lr / bc1) * (mi / denom)
    ei = ema * d + (p if mutant == "ema_old_p" else pi) * (one - d)
    assert all(a.dtype == np.float32 for a in (pi, mi, vi, ei))
    return dict(p=pi, m=mi, v=vi, ema=ei)


def _ratios(res, want, bound):
    return {k: float(((torch.from_numpy(res[k]).double() - want[k]).abs() / bound[k]).max()) for k in want}


def test_adamw_bounds_on_the_cpu():
    """No GPU: the fp32 restatement stays inside the bounds (and below 0.75 of them: they are not tight by accident), each mutant leaves
    them by a wide margin on the outputs it touches -- at every step of the GPU grid for which the mistake changes the rule."""
    cpu = torch.device("cpu")
    for step in (1, 2, 7, 1000):
        for wd in (0.0, 0.1):
            for coef in (1.0, 0.37):
                g = torch.Generator(cpu).manual_seed(step * 10 + int(wd * 10))
                inp = adamw_inputs(4099, step, g, cpu)
                h = dict(HYPER, wd=wd)
                want, bound = adamw_ref(*inp, h, step, coef)
                arrs = [t.numpy() for t in inp]
                r = _ratios(adamw_f32(*arrs, h, step, coef), want, bound)
                print(f"restatement step {step} wd {wd} coef {coef}: err / bound " + ", ".join(f"{k} {x:.3f}" for k, x in r.items()))
                assert all(x <= 0.75 for x in r.values()), r
                for mu in MUTANTS:
                    if (mu == "bc1_dropped" and step > 7) or (mu == "wd_without_lr" and wd == 0.0):
                        continue          # 1 - 0.9^1000 == 1;  wd == 0: nothing to scale
                    rm = _ratios(adamw_f32(*arrs, h, step, coef, mutant=mu), want, bound)
                    hit = "ema" if mu == "ema_old_p" else "p"
                    print(f"   mutant {mu}: {hit} err / bound {rm[hit]:.3g}")
                    assert rm[hit] > 100.0, (mu, step, wd, rm)


def _adamw_case(lib, dev, tag, n, step, via_dev, wd, stats_mode, with_ema, offsets, g):
    """One launch.  offsets: element offsets of (p, g, m, v, ema) inside their guarded buffers.  -> {name: err / bound}."""
    inp = adamw_inputs(n, step, g, dev)
    h = dict(HYPER, wd=wd)
    coef = 0.37 if stats_mode == "coef" else 1.0
    pairs = [_guarded(t, o) for t, o in zip(inp, offsets)]
    (pb, p), (gb, gr), (mb, m), (vb, v), (eb, ema) = pairs
    stats = None
    if stats_mode != "null":
        sbuf, stats = _guarded(torch.tensor([123.0, coef, 1.0 if stats_mode == "skip" else 0.0, SENT], device=dev))
    step_dev = None
    if via_dev:
        dbuf, step_dev = _guarded(torch.tensor([float(step)], device=dev))
    _call(lib, "latte_debug_adamw_ema", p, gr, m, v, ema if with_ema else None, n, h["lr"], h["b1"], h["b2"], h["eps"], wd,
          0 if via_dev else step, h["decay"], stats, step_dev)
    assert float(gr.abs().max()) == 0.0 and bool((gr.view(torch.int32) == 0).all()), f"{tag}: gradients not zeroed"
    got = dict(p=p, m=m, v=v, ema=ema)
    ratios = {}
    if stats_mode == "skip" or not with_ema:
        same = ("p", "m", "v", "ema") if stats_mode == "skip" else ("ema",)
        for k, t0 in zip(("p", "m", "v", "ema"), (inp[0], inp[2], inp[3], inp[4])):
            if k in same:
                assert torch.equal(got[k].view(torch.int32), t0.view(torch.int32)), f"{tag}: {k} changed"
    if stats_mode != "skip":
        want, bound = adamw_ref(*inp, h, step, coef)
        for k in ("p", "m", "v") + (("ema",) if with_ema else ()):
            ratios[k] = _within(f"{tag}: {k}", got[k], want[k], bound[k])
    for (buf, view), k in zip(pairs, ("p", "g", "m", "v", "ema")):
        _guards_intact(f"{tag}: {k}", buf, view)
    if stats is not None:
        assert stats.tolist()[:3] == [123.0, _f32(coef), 1.0 if stats_mode == "skip" else 0.0], f"{tag}: stats written"
        _guards_intact(f"{tag}: stats", sbuf, stats[:3])
    if via_dev:
        assert float(step_dev[0]) == float(step)
        _guards_intact(f"{tag}: step_dev", dbuf, step_dev)
    return ratios


def _worst(acc, r):
    for k, x in r.items():
        acc[k] = max(acc.get(k, 0.0), x)


@gpu
@pytest.mark.parametrize("via_dev", [0, 1], ids=["host_step", "step_dev"])
@pytest.mark.parametrize("step", [1, 2, 7, 1000])
def test_adamw_ema_one_step(lib, dev, step, via_dev):
    """The grid of the module docstring at n in {1, 3, 5, 4099}: below one float4, a vector part with tails of 3, 1 and 3."""
    g = torch.Generator(dev).manual_seed(1000 * via_dev + step)
    worst = {}
    for n in (1, 3, 5, 4099):
        for wd in (0.0, 0.1):
            for stats_mode in ("null", "coef", "skip"):
                for with_ema in (True, False):
                    tag = f"adamw n{n} step{step} {'dev' if via_dev else 'host'} wd{wd} stats {stats_mode} ema {with_ema}"
                    _worst(worst, _adamw_case(lib, dev, tag, n, step, via_dev, wd, stats_mode, with_ema, (0,) * 5, g))
    print(f"adamw_ema step {step} via {'step_dev' if via_dev else 'host'}: worst err / bound " + ", ".join(f"{k} {x:.3f}" for k, x in worst.items()))


# vector form past 8192 blocks x 256 float4 with a tail of 3; scalar form (every pointer one float off) past 8192 x 256 elements;
# only g off: a mixed alignment, which must take the scalar path (a float4 access at g would fault or shift the gradients by one)
@gpu
@pytest.mark.parametrize("n,offsets", [(8192 * 256 * 4 + 4 * 256 * 3 + 3, (0, 0, 0, 0, 0)), (8192 * 256 + 259, (1, 1, 1, 1, 1)),
                                       (4099, (0, 1, 0, 0, 0))], ids=["vector_past_cap", "scalar_past_cap", "mixed_alignment"])
def test_adamw_ema_sizes_and_alignment(lib, dev, n, offsets):
    g = torch.Generator(dev).manual_seed(n)
    worst = {}
    for step, via_dev, stats_mode, with_ema in ((7, 1, "coef", True), (2, 0, "skip", True), (1000, 0, "null", False)):
        tag = f"adamw n{n} offsets {offsets} step{step} stats {stats_mode} ema {with_ema}"
        _worst(worst, _adamw_case(lib, dev, tag, n, step, via_dev, 0.1, stats_mode, with_ema, offsets, g))
    print(f"adamw_ema n {n} offsets {offsets}: worst err / bound " + ", ".join(f"{k} {x:.3f}" for k, x in worst.items()))


@gpu
def test_adamw_ema_refuses(lib, dev):
    z = torch.zeros(8, device=dev)
    s = torch.ones(1, device=dev)
    call = lambda step, sd, p=z, n=8: _rc(lib, "latte_debug_adamw_ema", p, z.clone(), z.clone(), z.clone(), None, n, 1e-3, 0.9, 0.999, 1e-8,
                                          0.0, step, 0.99, None, sd)
    assert call(1, None) == 0 and call(0, s) == 0
    _sync(dev)
    for step, sd, kw in ((-1, None, {}), (-1, s, {}), (0, None, {}), (1, None, dict(p=None)), (1, None, dict(n=0))):
        assert call(step, sd, **kw) == LATTE_ERR_INVALID, (step, kw)


# ------------------------------------------------------------------------------------------------ gradient norm
def _ulps(a, b):
    return abs(int(np.float32(a).view(np.int32)) - int(np.float32(b).view(np.int32)))


def _grad_norm(lib, dev, gview, max_norm, clip, scaler=None):
    nb = lib.latte_debug_sumsq_blocks()
    # prefill -1: no sum of squares is negative (NaN would be a legitimate partial sum of a gradient that holds one)
    pbuf, partial = _guarded(torch.full((nb,), -1.0, device=dev, dtype=torch.float64), dtype=torch.float64)
    sbuf, stats = _guarded(torch.full((4,), SENT, device=dev))
    _call(lib, "latte_debug_grad_norm", gview, gview.numel(), partial, max_norm, clip, stats, scaler)
    out = stats.tolist()
    assert out[3] == SENT
    _guards_intact("grad_norm: stats", sbuf, stats[:3])
    assert not bool((partial == -1.0).any()), "grad_norm: a block wrote no partial sum"
    _guards_intact("grad_norm: partial", pbuf, partial)
    return out


@gpu
@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset1"])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 262144 + 5, 1048576 + 4 * 256 + 3])
def test_grad_norm(lib, dev, n, offset):
    """1024 blocks x 256 threads: 262144 + 5 passes one sweep of the scalar loop (which a g one float off 16 bytes takes entirely),
    1048576 + 4 x 256 + 3 one sweep of the 16-byte loop, with a tail of 3.  Magnitudes log-uniform in [1e-12, 1e12]: in an fp32
    accumulator the squares below 2^-24 of the running sum would vanish."""
    gen = torch.Generator(dev).manual_seed(n * 2 + offset)
    mag = 10.0 ** (torch.rand(n, generator=gen, device=dev, dtype=torch.float64) * 24 - 12)
    vals = (mag * torch.where(torch.rand(n, generator=gen, device=dev) < 0.5, -1.0, 1.0)).float()
    gbuf, gv = _guarded(vals, offset)
    assert (gv.data_ptr() % 16 == 0) == (offset == 0)
    ref = math.sqrt(float(np.sum(vals.cpu().numpy().astype(np.float64) ** 2)))
    worst = 0.0
    for factor, clip in ((1.001, 1), (0.999, 1), (0.999, 0), (0.5, 1)):
        max_norm = _f32(ref * factor)
        norm, coef, skip, _ = _grad_norm(lib, dev, gv, max_norm, clip)
        assert _ulps(norm, ref) <= 1, f"norm {norm!r} against {ref!r}: {_ulps(norm, ref)} ulp"
        raw = max_norm / (norm + _f32(1e-6))         # the kernel's 1e-6f is the fp32 nearest to 1e-6
        want = min(raw, 1.0) if clip else 1.0
        assert abs(coef - want) <= 2 * U32 * want, (factor, clip, coef, want)
        if abs(raw - 1.0) > 1e-4:                    # (a norm near 1e-3 puts the 1e-6 on the scale of the factor)
            assert (coef == 1.0) == (not clip or raw > 1.0), (factor, clip, coef, raw)
        assert skip == 0.0
        worst = max(worst, abs(coef - want) / (2 * U32 * want))
    assert torch.equal(gv, vals), "grad_norm: the gradients changed"
    _guards_intact("grad_norm: g", gbuf, gv)
    print(f"grad_norm n {n} offset {offset}: norm within {_ulps(norm, ref)} ulp, coefficient err / bound {worst:.3f}")


@gpu
@pytest.mark.parametrize("n", [5, 262144 + 5])
@pytest.mark.parametrize("kind", ["inf", "nan", "overflow"])
def test_grad_norm_not_finite(lib, dev, n, kind):
    """inf / nan at the first or the last element (vector part, scalar tail), or a finite fp64 sum whose root exceeds FLT_MAX."""
    for pos in (0, n - 1):
        vals = torch.full((n,), 1e-3, device=dev)
        if kind == "overflow":
            vals[pos] = 3e38
            vals[n // 2] = 3e38
        else:
            vals[pos] = float(kind)
        gbuf, gv = _guarded(vals)
        for clip in (0, 1):
            norm, coef, skip, _ = _grad_norm(lib, dev, gv, 1.0, clip)
            assert not math.isfinite(norm) and coef == 0.0 and skip == 1.0, (kind, pos, clip, norm, coef, skip)


@gpu
def test_grad_norm_refuses(lib, dev):
    z = torch.ones(8, device=dev)
    part = torch.zeros(lib.latte_debug_sumsq_blocks(), device=dev, dtype=torch.float64)
    st = torch.zeros(4, device=dev)
    call = lambda g=z, n=8, p=part, s=st, clip=1: _rc(lib, "latte_debug_grad_norm", g, n, p, 1.0, clip, s, None)
    assert call() == 0
    _sync(dev)
    for kw in (dict(g=None), dict(n=0), dict(p=None), dict(s=None), dict(clip=2)):
        assert call(**kw) == LATTE_ERR_INVALID, kw


# ------------------------------------------------------------------------------------------------ loss-scale state machine
def scaler_model(s, ok):
    """The comment above gradnorm_finalize_kernel, on a list of eight fp32 values."""
    f = np.float32
    s = [f(x) for x in s]
    if ok:
        s[2] += f(1)
        s[1] += f(1)
        s[4] = f(0)
        if s[5] != 0 and s[1] >= s[6]:
            s[0] = min(s[0] * f(2), s[7])
            s[1] = f(0)
    else:
        s[3] += f(1)
        s[4] = f(1)
        s[1] = f(0)
        if s[5] != 0:
            s[0] = max(s[0] * f(0.5), f(1))
    return [float(x) for x in s]


@gpu
def test_scaler_state_machine(lib, dev):
    """Nineteen calls from {scale 4, interval 2, cap 16}: two growths, the cap (a doubling that must stay at 16), a good step and then a
    skip that resets the growth count and leaves the applied updates alone, halvings 8 -> 4 -> 2 -> 1 and one more at the floor, growth
    again, then static mode (skips counted, scale fixed, the growth count running past the interval), then scaler == NULL.  All eight
    floats equal to the model's after every call."""
    fin = torch.full((37,), 0.25, device=dev)
    bad = fin.clone()
    bad[17] = float("inf")
    state = [4.0, 0.0, 0.0, 0.0, 0.0, 1.0, 2.0, 16.0]
    scbuf, sc = _guarded(torch.tensor(state, device=dev))
    script = [1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 1, 1] + ["static", 0, 1, 1, 1]
    seen = set()
    for i, ok in enumerate(script):
        if ok == "static":
            state[5] = 0.0
            sc[5] = 0.0
            continue
        before = list(state)
        state = scaler_model(state, ok)
        norm, coef, skip, _ = _grad_norm(lib, dev, fin if ok else bad, 1.0, 0, sc)
        assert skip == (0.0 if ok else 1.0) and coef == (1.0 if ok else 0.0)
        assert sc.tolist() == state, f"call {i} ({'finite' if ok else 'inf'}): {sc.tolist()} against the model's {state}"
        if ok and state[0] > before[0]:
            seen.add("growth")
        if ok and before[5] and before[1] + 1 >= before[6] and before[0] == before[7] and state[0] == before[7]:
            seen.add("cap")
        if not ok and before[1] > 0 and state[1] == 0 and state[2] == before[2]:
            seen.add("skip resets the growth count")
        if not ok and before[0] == 1.0 and before[5] and state[0] == 1.0:
            seen.add("floor")
        if not before[5] and not ok and state[0] == before[0]:
            seen.add("static skip")
        if not before[5] and ok and state[1] > state[6]:
            seen.add("static: no growth past the interval")
    assert seen == {"growth", "cap", "skip resets the growth count", "floor", "static skip", "static: no growth past the interval"}, seen
    norm, coef, skip, _ = _grad_norm(lib, dev, bad, 1.0, 1, None)          # no scaler: only the statistics
    assert skip == 1.0 and coef == 0.0 and sc.tolist() == state
    _guards_intact("scaler", scbuf, sc)
