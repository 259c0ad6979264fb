"""The training step's row kernels (csrc/train.hip) through their C-ABI hooks, at the widths and row counts training runs:
gated residual + next LayerNorm (forward), LayerNorm-modulate backward (plain and gated, dx_in absent / separate / in place), gated
residual backward, and the loss gradient.  Every hook is compared with an fp64 torch autograd reference on the same half-rounded
inputs.

Each comparison is local: row outputs per row, reduced outputs per (sample, column) or per partial row, so that one wrong run,
sample or chunk group fails even where a tensor-wide norm would not notice.  The bounds are first-order rounding-error bounds built
from the operand type's unit roundoff (outputs rounded to bf16 / f16), fp32's unit roundoff times the longest chain of fp32
operations behind a value, and the row's conditioning (|mean| / std of a LayerNorm row; the cancellations of the loss terms),
each evaluated in fp64 on the same inputs.  None of them is a measured number."""
import math

import pytest
import torch

from latte_amd._lib import check, ptr, stream_ptr

pytestmark = pytest.mark.gpu
TD = {"bf16": torch.bfloat16, "f16": torch.float16}
DT = {"bf16": 0, "f16": 1}
U_OUT = {"bf16": 2.0 ** -9, "f16": 2.0 ** -11}   # unit roundoff of the half output
ETA = {"bf16": 0.0, "f16": 2.0 ** -25}           # absolute rounding error of an f16 subnormal (dy of 1e-6 ... 1e-4 lands there)
U32 = 2.0 ** -24
LATTE_ERR_INVALID = 1

DS = [128, 384, 768, 1024, 1152, 1280]   # 3 / 5 chunk groups per lane, full and partial last groups, the 1280 bound
RPS = [64, 128, 4096]                    # 2, 4 and 128 partial rows per sample
SAMPLES = [1, 3, 9]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda")


def _chain(D):
    """fp32 operations behind a row statistic: NQ chunk groups x 4 lanes per lane, the 6-level wave butterfly, the divide and sqrt."""
    return 4 * math.ceil(D / 256) + 6 + 4


def _rows(M, D, rps, g, dev):
    """LayerNorm input rows of three kinds: ordinary rows (std 0.5 ... 2, mean within +-1), every 7th row with a large common offset
    (|mean| / std = 100), every 11th row near-constant (variance 1e-10, far below the LayerNorm eps 1e-6)."""
    r = torch.arange(M, device=dev)
    sig = 0.5 + 1.5 * torch.rand(M, 1, generator=g, device=dev, dtype=torch.float64)
    mu = torch.rand(M, 1, generator=g, device=dev, dtype=torch.float64) * 2 - 1
    n = torch.randn(M, D, generator=g, device=dev, dtype=torch.float64)
    x = mu + sig * n
    off = (r % 7 == 3)[:, None]
    const = (r % 11 == 5)[:, None]
    x = torch.where(off, 100.0 + n, x)
    x = torch.where(const, mu + 1e-5 * n, x)
    return x.float(), off.squeeze(1), const.squeeze(1)


def _modulation(S, D, g, dev):
    """shift N(0, 1); scale N(0, 0.5), with every third column at -1 + 1e-3 N(0, 1) (the (1 + scale) factor near zero)."""
    shift = torch.randn(S, D, generator=g, device=dev)
    scale = 0.5 * torch.randn(S, D, generator=g, device=dev)
    near = torch.arange(D, device=dev) % 3 == 0
    scale[:, near] = -1.0 + 1e-3 * torch.randn(S, int(near.sum()), generator=g, device=dev)
    return shift, scale


EPS = 1e-6   # the LayerNorm eps of latte.py (elementwise_affine=False, eps=1e-6)


def _xhat_err(x):
    """absolute error bound of the kernel's xhat = (x - mean) rstd per element, [M, D]: the mean's fp32 sum errs by ~chain u |mean|,
    which rstd = 1 / sqrt(var + eps) scales (the row's conditioning kappa = 1 + |mean| rstd), and rstd's own relative error scales
    xhat.  With the eps inside: near-constant rows (variance << eps) have kappa ~ 1e3, not |mean| / std ~ 1e5."""
    x = x.double()
    D = x.shape[1]
    rstd = 1.0 / torch.sqrt(x.var(1, unbiased=False, keepdim=True) + EPS)
    kappa = 1.0 + x.mean(1, keepdim=True).abs() * rstd
    xhat = (x - x.mean(1, keepdim=True)) * rstd
    return U32 * _chain(D) * (kappa + xhat.abs())


def _check_rows(name, got, want, bound, rps, slack=2.0):
    """per row: ||got_r - want_r|| <= slack * ||bound_r||; the message names the row, its sample and its worst chunk group."""
    err = got.double() - want
    en = err.norm(dim=1)
    bn = bound.norm(dim=1)
    bad = ~(en <= slack * bn)
    if bool(bad.any()):
        r = int(torch.nonzero(bad)[0])
        D = err.shape[1]
        col = int(err[r].abs().argmax())
        raise AssertionError(f"{name}: {int(bad.sum())} of {err.shape[0]} rows out of bound; first row {r} (sample {r // rps}, column "
                             f"{col}, chunk group {col // 256} of {math.ceil(D / 256)}): err {float(en[r]):.3e} > {slack} x {float(bn[r]):.3e}"
                             f", |want_r| {float(want[r].norm()):.3e}")
    return float((en / bn.clamp_min(1e-300)).max())


def _check_elems(name, got, want, bound, slack=2.0):
    """per element (the reduced outputs: per sample and column, per partial row and column)."""
    err = (got.double() - want).abs()
    bad = ~(err <= slack * bound)
    if bool(bad.any()):
        idx = tuple(int(i) for i in torch.nonzero(bad)[0])
        raise AssertionError(f"{name}: {int(bad.sum())} of {err.numel()} elements out of bound; first {idx}: err {float(err[idx]):.3e} > "
                             f"{slack} x {float(bound[idx]):.3e}, want {float(want[idx]):.3e}")


def _dy_rows(M, D, g, dev, dt, const):
    """upstream gradient rows spanning the loss-scaled range: each row scaled by 10^U(-6, 3) (near-constant rows, whose rstd is
    ~1e3, by 10^U(-6, 0) so that their dx stays inside f16's range), rounded to the operand type."""
    lg = torch.rand(M, 1, generator=g, device=dev, dtype=torch.float64) * 9 - 6
    lg = torch.where(const[:, None], lg * (6.0 / 9.0) - 2.0, lg)
    return (torch.randn(M, D, generator=g, device=dev, dtype=torch.float64) * 10.0 ** lg).to(TD[dt])


def _case_id(D, rps, S, dt):
    return f"D{D}-rps{rps}-S{S}-{dt}"


GRID = [(D, rps, S, dt) for dt in ("bf16", "f16") for D in DS for rps in RPS for S in SAMPLES]


# ------------------------------------------------------------------------------------------------ gated residual + next LayerNorm
@pytest.mark.parametrize("D,rps,S,dt", GRID, ids=[_case_id(*c) for c in GRID])
def test_gated_add_ln(lib, dev, D, rps, S, dt):
    M = rps * S
    g = torch.Generator(dev).manual_seed(D * 7919 + rps * 31 + S)
    xo, off, const = _rows(M, D, rps, g, dev)
    gate = torch.randn(S, 6 * D, generator=g, device=dev)
    shift, scale = _modulation(S, D, g, dev)
    mod = torch.cat([gate[:, :D], shift, scale, gate[:, D:4 * D]], 1).contiguous()   # gate | shift | scale at a stride of 6 D
    y = torch.randn(M, D, generator=g, device=dev).to(TD[dt])
    y[const] = 0
    smp = torch.arange(M, device=dev) // rps
    T = 16 if rps % 16 == 0 else 1
    F = rps // T
    te = torch.randn(F, D, generator=g, device=dev)
    frame = (torch.arange(M, device=dev) // T) % F
    u = U_OUT[dt]
    for use_te in (False, True):
        ted = te.double()[frame] if use_te else torch.zeros(M, D, device=dev, dtype=torch.float64)
        gy = mod[smp, :D].double() * y.double()
        x_in = (xo.double() - gy - ted).float()        # x_out lands on the designed rows (offset, near-constant) to fp32 rounding
        x_out = torch.empty(M, D, device=dev)
        xn = torch.empty(M, D, device=dev, dtype=TD[dt])
        check(lib.latte_debug_gated_add_ln(ptr(x_in), ptr(y), ptr(mod), 6 * D, ptr(x_out), ptr(xn), ptr(mod[:, D:]), ptr(mod[:, 2 * D:]), 6 * D,
                                           M, D, rps, ptr(te) if use_te else None, T, F, DT[dt], stream_ptr()))
        torch.cuda.synchronize()
        want_x = x_in.double() + gy + ted
        # x_out: at most one rounding per addition
        _check_elems("x_out", x_out, want_x, 2 * U32 * (x_in.double().abs() + gy.abs() + ted.abs()), slack=1.0)
        xr = want_x
        xhat = torch.nn.functional.layer_norm(xr, (D,), eps=EPS)
        sc, sh = mod[smp, 2 * D:3 * D].double(), mod[smp, D:2 * D].double()
        want = xhat * (1 + sc) + sh
        # the statistics' error reaches xn through (1 + scale) only; the shift is one fp32 add (and the fp32 x_out rounding, 2 u)
        bound = u * want.abs() + ETA[dt] + _xhat_err(xr) * (1 + sc).abs() + 2 * U32 * (want.abs() + sh.abs())
        _check_rows(f"xn (te={use_te})", xn, want, bound, rps)


# ------------------------------------------------------------------------------------------------ LayerNorm-modulate backward
def _ln_bwd_ref(x, dy, sc, dx_in):
    """fp64 autograd of y = LN(x) (1 + scale) + shift -> (dx + dx_in, xhat, per-element error bound of the kernel's dx, of its xhat).

    The kernel evaluates dx = rstd (dxhat - m1 - xhat m2) + dx_in, dxhat = dy (1 + scale), m1 = mean(dxhat), m2 = mean(dxhat xhat);
    first-order error: a few roundings on each product and difference, the wave sums' chain on m1 / m2, xhat's error (_xhat_err)
    through the xhat m2 term and through m2, rstd's relative error on the whole, one rounding of the dx_in add."""
    xd = x.double().requires_grad_(True)
    D = x.shape[1]
    xhat = torch.nn.functional.layer_norm(xd, (D,), eps=EPS)
    yv = xhat * (1 + sc)
    (dx,) = torch.autograd.grad(yv, xd, dy.double())
    xhat = xhat.detach()
    ex = _xhat_err(x)
    rstd = 1.0 / torch.sqrt(x.double().var(1, unbiased=False, keepdim=True) + EPS)
    dxh = dy.double() * (1 + sc)
    m1 = dxh.mean(1, keepdim=True)
    m2 = (dxh * xhat).mean(1, keepdim=True)
    chain = _chain(D)
    core = dxh.abs() + m1.abs() + xhat.abs() * m2.abs()
    err = rstd * (4 * U32 * core + chain * U32 * (dxh.abs().mean(1, keepdim=True) + xhat.abs() * (dxh * xhat).abs().mean(1, keepdim=True))
                  + ex * m2.abs() + xhat.abs() * (dxh.abs() * ex).mean(1, keepdim=True)) + (chain + 1) * U32 * dx.detach().abs()
    if dx_in is not None:
        dx = dx + dx_in.double()
        err = err + U32 * (dx.abs() + dx_in.double().abs())
    return dx, xhat, err, ex


def _sample_sums(v, rps):
    M, D = v.shape
    return v.view(M // rps, rps, D).sum(1)


FORMS = ["plain", "gated_inplace", "separate_dx_in"]
LN_GRID = [(D, rps, S, dt, f) for (D, rps, S, dt) in GRID for f in FORMS
           if f != "separate_dx_in" or (S == 3 and rps != 4096)]


@pytest.mark.parametrize("D,rps,S,dt,form", LN_GRID, ids=[_case_id(*c[:4]) + "-" + c[4] for c in LN_GRID])
def test_ln_bwd(lib, dev, D, rps, S, dt, form):
    """plain: dx_in NULL, dshift / dscale through the finalize kernel (128 partial rows per sample at 4096 rows).  gated_inplace: what
    train_engine.cpp does between two blocks -- dx_in == dx_out, the gated residual's backward of the branch below on the same pass
    (dy2, and the partial rows of sum dx * y2 and sum gate2 * dx per 32 rows).  separate_dx_in: dx_in and dx_out distinct."""
    M = rps * S
    g = torch.Generator(dev).manual_seed(D * 104729 + rps * 17 + S * 3 + FORMS.index(form))
    x, off, const = _rows(M, D, rps, g, dev)
    shift, scale = _modulation(S, D, g, dev)
    mod = torch.cat([shift, scale, torch.randn(S, 4 * D, generator=g, device=dev)], 1).contiguous()
    smp = torch.arange(M, device=dev) // rps
    dy = _dy_rows(M, D, g, dev, dt, const)
    sc = mod[smp, D:2 * D].double()
    u = U_OUT[dt]
    ws = torch.full((M // 32 * 2 * D,), float("nan"), device=dev)
    dx_in = None
    if form != "plain":
        dx_in = torch.randn(M, D, generator=g, device=dev) * 10.0 ** (torch.rand(M, 1, generator=g, device=dev) * 6 - 4)
    want_dx, xhat, bound_dx, ex = _ln_bwd_ref(x, dy, sc, dx_in)
    dx_out = dx_in.clone() if form == "gated_inplace" else torch.full((M, D), float("nan"), device=dev)
    dsh = torch.full((S, D + 8), float("nan"), device=dev)
    dsc = torch.full((S, D + 8), float("nan"), device=dev)
    y2 = gate2 = dy2 = gp = None
    if form == "gated_inplace":
        y2 = torch.randn(M, D, generator=g, device=dev).to(TD[dt])
        gate2 = mod[:, 2 * D:3 * D]
        dy2 = torch.empty(M, D, device=dev, dtype=TD[dt])
        gp = torch.full((M // 32, 2, D), float("nan"), device=dev)
    src = dx_out if form == "gated_inplace" else dx_in
    check(lib.latte_debug_ln_bwd(ptr(dy), ptr(x), ptr(mod[:, D:]), 6 * D, ptr(src), ptr(dx_out), ptr(dsh), ptr(dsc), D + 8, M, D, rps,
                                 ptr(y2), ptr(gate2), 6 * D, ptr(dy2), ptr(gp), ptr(ws), ws.numel(), DT[dt], stream_ptr()))
    torch.cuda.synchronize()
    _check_rows("dx", dx_out, want_dx, bound_dx, rps)
    # per-sample modulation gradients: sums over the sample's rows; each term carries xhat's error, the sum its fp32 chain
    # (8 rows per wave, 3 LDS adds, rps / 128 partial rows per finalize thread row, 2 final adds)
    red_chain = 8 + 3 + rps // 128 + 2
    dyd = dy.double()
    _check_elems("dshift", dsh[:, :D], _sample_sums(dyd, rps), U32 * red_chain * _sample_sums(dyd.abs(), rps))
    _check_elems("dscale", dsc[:, :D], _sample_sums(dyd * xhat, rps),
                 _sample_sums(dyd.abs() * (xhat.abs() * U32 * (red_chain + 1) + ex), rps))
    if form == "gated_inplace":
        g2 = gate2[smp].double()
        want_dy2 = g2 * want_dx
        _check_rows("dy2", dy2, want_dy2, u * want_dy2.abs() + ETA[dt] + g2.abs() * bound_dx, rps)
        y2d = y2.double()
        blk = lambda v: v.view(M // 32, 32, D).sum(1)
        _check_elems("gpartial[sum dx y2]", gp[:, 0], blk(want_dx * y2d),
                     blk((want_dx * y2d).abs() * U32 * 12 + y2d.abs() * bound_dx))
        _check_elems("gpartial[sum gate2 dx]", gp[:, 1], blk(g2 * want_dx),
                     blk((g2 * want_dx).abs() * U32 * 12 + g2.abs() * bound_dx))


# ------------------------------------------------------------------------------------------------ gated residual backward
GATE_GRID = [(D, rps, S, dt, bp) for (D, rps, S, dt) in GRID for bp in (0, 1) if bp == 0 or S != 1]


@pytest.mark.parametrize("D,rps,S,dt,bias_partial", GATE_GRID, ids=[_case_id(*c[:4]) + f"-bias{c[4]}" for c in GATE_GRID])
def test_gate_bwd(lib, dev, D, rps, S, dt, bias_partial):
    """dy = gate * dx (half), dgate per sample through the finalize kernel, and (bias_partial 1) the partial rows of sum gate * dx."""
    M = rps * S
    g = torch.Generator(dev).manual_seed(D * 15485863 + rps * 13 + S * 5 + bias_partial)
    dx = torch.randn(M, D, generator=g, device=dev) * 10.0 ** (torch.rand(M, 1, generator=g, device=dev) * 9 - 6)
    y = torch.randn(M, D, generator=g, device=dev).to(TD[dt])
    gate = torch.randn(S, 6 * D, generator=g, device=dev)
    gate[:, 1::5] = -1.0 + 1e-3 * torch.randn(S, gate[:, 1::5].shape[1], generator=g, device=dev)
    smp = torch.arange(M, device=dev) // rps
    ns = 1 + bias_partial
    part = torch.full((M // 32, ns, D), float("nan"), device=dev)
    dy = torch.empty(M, D, device=dev, dtype=TD[dt])
    dg = torch.full((S, D + 4), float("nan"), device=dev)
    check(lib.latte_debug_gate_bwd(ptr(dx), ptr(y), ptr(gate[:, 2 * D:]), 6 * D, ptr(dy), ptr(part), part.numel(), ptr(dg), D + 4, M, D, rps,
                                   bias_partial, DT[dt], stream_ptr()))
    torch.cuda.synchronize()
    gd = gate[smp, 2 * D:3 * D].double()
    dxd, yd = dx.double(), y.double()
    want_dy = gd * dxd
    _check_rows("dy", dy, want_dy, U_OUT[dt] * want_dy.abs() + ETA[dt] + U32 * want_dy.abs(), rps)
    red_chain = 8 + 3 + rps // 128 + 2
    _check_elems("dgate", dg[:, :D], _sample_sums(dxd * yd, rps), U32 * (red_chain + 1) * _sample_sums((dxd * yd).abs(), rps))
    blk = lambda v: v.view(M // 32, 32, D).sum(1)
    _check_elems("partial[sum dx y]", part[:, 0], blk(dxd * yd), U32 * 12 * blk((dxd * yd).abs()))
    if bias_partial:
        _check_elems("partial[sum gate dx]", part[:, 1], blk(want_dy), U32 * 12 * blk(want_dy.abs()))


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("D,rps,why", [(1284, 64, "D > 1280"), (130, 64, "D % 4"), (128, 48, "rows per sample % 32"),
                                       (128, 16, "rows per sample % 32"), (384, 80, "rows per sample % 32")])
def test_row_kernels_refuse_shapes_they_cannot_take(lib, dev, D, rps, why):
    """LATTE_ERR_INVALID and nothing written.  (Every buffer is sized for the requested shape, so even a launch could not reach past
    it.)"""
    S = 2
    M = rps * S
    x = torch.randn(M, D, device=dev)
    h = torch.randn(M, D, device=dev).to(torch.float16)
    mod = torch.randn(S, 6 * D, device=dev)
    out = torch.full((M, D), 7.0, device=dev)
    hout = torch.full((M, D), 7.0, device=dev, dtype=torch.float16)
    ws = torch.full((M * 4 * D,), 7.0, device=dev)
    red = torch.full((S, D), 7.0, device=dev)

    def untouched():
        torch.cuda.synchronize()
        return bool((out == 7).all() and (hout == 7).all() and (ws == 7).all() and (red == 7).all())
    rc = lib.latte_debug_ln_bwd(ptr(h), ptr(x), ptr(mod), 6 * D, None, ptr(out), ptr(red), ptr(red), D, M, D, rps, None, None, 0, None, None,
                                ptr(ws), ws.numel(), 1, stream_ptr())
    assert rc == LATTE_ERR_INVALID and untouched(), (why, rc)
    rc = lib.latte_debug_ln_bwd(ptr(h), ptr(x), ptr(mod), 6 * D, ptr(x), ptr(out), None, None, D, M, D, rps, ptr(h), ptr(mod), 6 * D,
                                ptr(hout), ptr(ws[M * 2 * D:]), ptr(ws), M * 2 * D, 1, stream_ptr())
    assert rc == LATTE_ERR_INVALID and untouched(), (why, rc)
    rc = lib.latte_debug_gate_bwd(ptr(x), ptr(h), ptr(mod), 6 * D, ptr(hout), ptr(ws), ws.numel(), ptr(red), D, M, D, rps, 1, 1, stream_ptr())
    assert rc == LATTE_ERR_INVALID and untouched(), (why, rc)
    if D % 4 or D > 1280:      # the forward row kernel takes any whole number of rows per sample
        rc = lib.latte_debug_gated_add_ln(ptr(x), ptr(h), ptr(mod), 6 * D, ptr(out), ptr(hout), ptr(mod), ptr(mod), 6 * D, M, D, rps, None,
                                          1, 1, 1, stream_ptr())
        assert rc == LATTE_ERR_INVALID and untouched(), (why, rc)


# ------------------------------------------------------------------------------------------------ loss gradient
def _loss_grad_bound(s, x0, xt, mo, t, C):
    """first-order bound of the fp32 kernel's error on the variance channels: sum over the fp32 intermediates z of
    |d dmo / d z| * (error of z), the partial derivatives by fp64 autograd of the kernel's own expression of the gradient."""
    from oracle.diffusion_oracle import _coef_t
    nd = x0.dim()
    c = 8 * U32
    f = lambda arr: _coef_t(arr, t, nd).double()
    coef1, coef2 = f(s.posterior_mean_coef1), f(s.posterior_mean_coef2)
    plv, lb = f(s.posterior_log_variance_clipped), f(s.log_betas)
    srec, srecm1 = f(s.sqrt_recip_alphas_cumprod), f(s.sqrt_recipm1_alphas_cumprod)
    xs, xv = x0.double(), xt.double()
    pred, v = mo[:, :, :C].double(), mo[:, :, C:].double()
    x0p = pred if s.predict_xstart else srec * xv - srecm1 * pred
    d_x0p = 0 * pred if s.predict_xstart else c * (srec * xv).abs() + c * (srecm1 * pred).abs()
    mean = coef1 * x0p + coef2 * xv
    d_mean = c * ((coef1 * x0p).abs() + (coef2 * xv).abs()) + coef1.abs() * d_x0p
    lv = ((v + 1) / 2 * lb + (1 - (v + 1) / 2) * plv)
    d_lv = c * ((v + 1).abs() / 2 * lb.abs() + (1 - v).abs() / 2 * plv.abs())
    k = 0.5 * (lb - plv)
    # KL branch:  dlv = 0.5 (1 - e^(plv - lv) - dm^2 e^-lv),  dm = (coef1 xs + coef2 xv) - mean
    lvk = lv.clone().requires_grad_(True)
    dmk = ((coef1 * xs + coef2 * xv) - mean).requires_grad_(True)
    dkl = 0.5 * (1 - torch.exp(plv - lvk) - dmk * dmk * torch.exp(-lvk))
    g_lv, g_dm = torch.autograd.grad(dkl.sum(), [lvk, dmk])
    d_dm = c * ((coef1 * xs).abs() + (coef2 * xv).abs() + mean.abs()) + d_mean
    b_kl = g_lv.abs() * d_lv + g_dm.abs() * d_dm + c * (1 + torch.exp(plv - lv) + dmk.detach() ** 2 * torch.exp(-lv))
    # decoder-NLL branch (t == 0): the selected log-probability's derivative in the kernel's form, as a function of the cdf
    # arguments and of the cdf / cdf-derivative values (each a tanh in fp32: absolute error ~ u on the cdf, relative ~ u on its slope)
    inv = torch.exp(-0.5 * lv)
    centered = xs - mean
    a = math.sqrt(2 / math.pi)
    cdf = lambda p: 0.5 * (1 + torch.tanh(a * (p + 0.044715 * p ** 3)))
    slope = lambda p: 0.5 * (1 - torch.tanh(a * (p + 0.044715 * p ** 3)) ** 2) * a * (1 + 0.134145 * p * p)
    sel_lo, sel_hi = xs < -0.999, xs > 0.999

    def dnll_of(pin, pmn, cp, cm, gp, gm):
        # the kernel's branches; denominators made safe where a branch is not selected (no inf * 0 in the derivatives)
        ok_lo, ok_hi, ok_mid = cp > 1e-12, 1 - cm > 1e-12, cp - cm > 1e-12
        lo = torch.where(ok_lo, gp * (-pin) / torch.where(ok_lo, cp, 1.0), 0 * cp)
        hi = torch.where(ok_hi, -gm * (-pmn) / torch.where(ok_hi, 1 - cm, 1.0), 0 * cm)
        mid = torch.where(ok_mid, (gp * (-pin) - gm * (-pmn)) / torch.where(ok_mid, cp - cm, 1.0), 0 * cp)
        return -0.5 * torch.where(sel_lo, lo, torch.where(sel_hi, hi, mid))

    p_in = (inv * (centered + 1 / 255.0)).requires_grad_(True)
    p_mn = (inv * (centered - 1 / 255.0)).requires_grad_(True)
    dnll = dnll_of(p_in, p_mn, cdf(p_in), cdf(p_mn), slope(p_in), slope(p_mn))
    g_pin, g_pmn = torch.autograd.grad(dnll.sum(), [p_in, p_mn])            # through the cdf and its slope as well
    pin, pmn = p_in.detach(), p_mn.detach()
    leaves = [cdf(pin).requires_grad_(True), cdf(pmn).requires_grad_(True), slope(pin).requires_grad_(True), slope(pmn).requires_grad_(True)]
    g_cp, g_cm, g_gp, g_gm = torch.autograd.grad(dnll_of(pin, pmn, *leaves).sum(), leaves)
    gp, gm = leaves[2].detach(), leaves[3].detach()
    d_p = lambda p: c * p.abs() * (1 + lv.abs()) + inv * (c * (xs.abs() + mean.abs()) + d_mean)
    b_nll = (g_pin.abs() * d_p(pin) + g_pmn.abs() * d_p(pmn) + (g_cp.abs() + g_cm.abs()) * 4 * U32
             + g_gp.abs() * c * gp + g_gm.abs() * c * gm + c * dnll.detach().abs())
    t0 = (t == 0).view(-1, *([1] * (nd - 1)))
    return (torch.where(t0, b_nll, b_kl) * k.abs() + c * 2 * (torch.where(t0, dnll, dkl).detach() * k).abs()).detach()


LOSS_GRID = [("", 0, True), ("", 0, False), ("250", 1, True), ("250", 0, True)]


@pytest.mark.parametrize("spec,loss_type,learn_sigma", LOSS_GRID, ids=[f"steps{c[0] or 1000}-loss{c[1]}-sigma{int(c[2])}" for c in LOSS_GRID])
def test_loss_grad(lib, dev, spec, loss_type, learn_sigma):
    """d mean(terms["loss"]) / d model_output against fp64 autograd of the oracle's loss (gaussian_diffusion.py:719-795), at config 5's
    sample shape (16 frames x 4 x 32 x 32) with t at 0, 1, mid and last, x0 drawn like scaled latents (N(0, 1), NOT clamped to
    [-1, 1]: the decoder NLL's three branches all run) and trained-model-like outputs (eps N(0, 1), v in [-1, 1])."""
    import latte_amd
    from oracle import diffusion_oracle as do
    s = do.Schedule(spec, learn_sigma=learn_sigma)
    d = latte_amd.create_diffusion(spec, learn_sigma=learn_sigma, rescale_learned_sigmas=loss_type == 1)
    n = s.num_timesteps
    t = torch.tensor([0, 1, n // 2, n - 1, 0, n - 1])
    B, F, C, H = t.shape[0], 16, 4, 32
    g = torch.Generator().manual_seed(1000 + LOSS_GRID.index((spec, loss_type, learn_sigma)))
    x0 = torch.randn(B, F, C, H, H, generator=g)
    noise = torch.randn(B, F, C, H, H, generator=g)
    xt = do.q_sample(s, x0, t, noise)
    eps = noise + 0.3 * torch.randn(B, F, C, H, H, generator=g)
    mo = torch.cat([eps, torch.rand(B, F, C, H, H, generator=g) * 2 - 1], 2) if learn_sigma else eps
    # reference: fp64 autograd of the oracle's terms on the same fp32 inputs
    mod = mo.double().requires_grad_(True)
    terms = {}
    if learn_sigma:
        frozen = torch.cat([mod[:, :, :C].detach(), mod[:, :, C:]], 2)
        terms["vb"] = do._vb_terms_bpd(s, frozen, x0.double(), xt.double(), t) * (n / 1000.0 if loss_type == 1 else 1.0)
    terms["mse"] = do._mean_flat((noise.double() - mod[:, :, :C]) ** 2)
    loss = (terms["mse"] + terms.get("vb", 0)).mean()
    (want,) = torch.autograd.grad(loss, mod)
    got = torch.full(mo.shape, float("nan"), device=dev)
    args = [x.contiguous().to(dev) for x in (x0, xt, noise, mo)]
    t_dev = t.to(dev)
    check(lib.latte_debug_loss_grad(d._h, loss_type, *[ptr(a) for a in args], ptr(t_dev), B, F, C, H * H, ptr(got), stream_ptr()))
    torch.cuda.synchronize()
    got = got.cpu().double()
    # eps channels: 2 (pred - target) / (per batch): three fp32 roundings
    _check_elems("d eps", got[:, :, :C], want[:, :, :C], 4 * U32 * want[:, :, :C].abs() + 1e-30)
    if learn_sigma:
        per = F * C * H * H
        wvb = (n / 1000.0 if loss_type == 1 else 1.0) / (per * B * math.log(2.0))
        bound = _loss_grad_bound(s, x0, xt, mo, t, C) * wvb
        bound = bound + 4 * U32 * want[:, :, C:].abs()
        _check_elems("d v", got[:, :, C:], want[:, :, C:], bound)
        # all three decoder-NLL branches were taken, with a non-zero gradient in each
        nz = (want[:, :, C:].abs() > 0)[t == 0]
        xs0 = x0[t == 0]
        for sel in (xs0 < -0.999, xs0 > 0.999, xs0.abs() <= 0.999):
            assert int((nz & sel).sum()) > 100
