"""The VAE's GroupNorm (csrc/vae.hip: gn_partial_kernel, gn_finalize_kernel, gn_apply_kernel) through latte_debug_groupnorm_ex, which
exposes the launcher's eps, max_slabs and y_lo and reads the statistics back: the statistics pass and the apply pass are checked
separately, per (sample, group) and per element, against fp64.  u = 2^-24 throughout.

STATISTICS.  slabs = min(max(HW / 256, 1), max_slabs) workgroups per sample, per = ceil(HW / slabs) pixels each.  A thread owns one channel
octet and every px-th pixel of the slab (px = 2048 / C pixel lanes) and keeps one (sum, sum of squares) pair per half octet.  Per pixel its
`add` forms f0 + f1 (one rounding), adds it to the running sum (one), then the same for f2 + f3: an element passes 1 + 2 it roundings of the
serial chain, it = ceil(per / px).  The pixel-lane pass adds the px per-thread sums in lane order (px roundings), the column pass the
cpc = C / 128 half-octet columns of a group (cpc).  The squares carry one rounding more (the product; with contraction one of each pair
is exact, the count covers both forms).  gn_finalize adds the slabs in fp64: counted as exact.  With n = 1 + 2 it + px + cpc, count =
HW C / 32 and the sums taken over a (sample, group):

    dmean  <= n u sum|x| / count                    dE[x^2] <= (n + 1) u sum x^2 / count
    dvar    = dE[x^2] + 2 |mean| dmean + dmean^2    (var = E[x^2] - mean^2, the un-centred form the kernel uses)
    drstd   = 1/2 rstd^3 dvar                       and one fp32 rounding each of the stored mean and rstd: + u |mean|, + u rstd.

APPLY.  t = (x - mean) rstd gamma + beta is a subtraction, a product and one fused multiply-add (v_pk_fma_f32) on the kernel's OWN
statistics, which the reference therefore takes from the read-back: |dt| <= 4 u (|(x - mean) rstd gamma| + |beta|), one u per operation
on the product term and one on the sum.  SiLU = t / (1 + __expf(-t)): the fast exponential multiplies by log2(e) (the constant and the
product: 2 u |t| relative in the result) and takes v_exp_f32 (one ulp = 2 u), the sum and the correctly rounded division add u each, and
the exponential's error reaches the result scaled by sigmoid(-t): relative u (4 + 2 |t| sigmoid(-t)); dt goes through |dSiLU/dt| <= 1.1.
The stored y is one f16 rounding of that: 2^-11 |y|, with the f16 subnormal spacing 2^-24 as floor.

y_lo = f16(o - y), o the fp32 value before the rounding.  y must not change when y_lo is asked for (compared bit for bit).  o - y is exact
in fp32 and at most 2^-11 |o|, so its f16 rounding leaves |(y + y_lo) - want| <= dt + 2^-22 |want| -- where the residual is a normal f16
number.  Below 2^-14 (every |o| < 1/8) the residual lands among the f16 subnormals and its rounding error is half their spacing, 2^-25,
whatever |want|: the bound carries that floor, max(2^-22 |want|, 2^-25).  For silu = 0 the fp32 restatement below is the kernel operation
for operation, so y_lo must EQUAL f16(o - y) bit for bit wherever the restated o rounds to the y the kernel stored (elsewhere o is
ambiguous: skipped, at most 1 % of a case; the CPU half checks that the restatement's own ambiguity, the double rounding of the emulated
fused multiply-add, stays far below that).  With SiLU the fast exponential leaves o ambiguous in its last place at most elements, so only
the sum bound is asserted there.

INPUTS.  Every (sample, group) has its own sigma in [1/4, 4] and mean = +-offset sigma, offset in {0, 4, 32}; the eps cases give group 5 the
variance 1e-5, where eps = 1e-5 and 1e-6 differ by a quarter of rstd.  y and y_lo are NaN before every launch and lie between guard rows.

RECORDED, not asserted: the worst deviation of y from the TRUE fp64 GroupNorm (fp64 statistics) in f16 ulps, per offset -- what the
un-centred sums cost at |mean| / sigma = 32.  Two figures: in ulps of the element itself, which outputs near zero
(gamma t cancelling beta) dominate, and the worst absolute deviation in ulps of an output of magnitude 1 (2^-10).

The CPU half (not marked gpu) runs the restatement through the same checks on the same cases (up to 300 slabs) and shows that three named
mistakes leave the bounds."""
import math

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu
U32 = 2.0 ** -24
U16 = 2.0 ** -11
SUB16 = 2.0 ** -24          # spacing of the f16 subnormals
SENT = -7.25
GUARD = 3                   # guard rows of C halfs before and behind y / y_lo
LATTE_ERR_INVALID = 1


def _f32(v):
    return float(np.float32(v))


# (N, HW, C, x_is_f32, silu, eps, max_slabs, offset); slabs = min(max(HW // 256, 1), max_slabs)
def _cases():
    out = []
    hw128 = [(3, 100), (1, 511), (2, 2 * 256), (1, 7 * 256 + 13), (1, 8 * 256), (3, 9 * 256 + 255), (1, 24 * 256 + 1), (1, 25 * 256),
             (1, 26 * 256 + 100), (1, 32 * 256), (2, 33 * 256 + 7), (1, 57 * 256 + 201), (1, 256 * 256)]
    for i, (N, HW) in enumerate(hw128):
        out.append((N, HW, 128, i % 2, (i // 2) % 2, 1e-6 if i % 3 else 1e-5, 256, (0, 4, 32)[i % 3]))
    out.append((1, 300 * 256 + 77, 128, 1, 1, 1e-5, 512, 32))            # the temporal form: one sample, more than 256 slabs
    out.append((1, 1025 * 256 + 37, 128, 0, 1, 1e-5, 256 * 14, 4))
    for C in (256, 512):
        for j, s in enumerate((1, 9, 33)):
            out.append((1 + 2 * (j == 1), s * 256 + (0, 131, 255)[j], C, (j + C // 256) % 2, j % 2, 1e-5 if j == 1 else 1e-6, 256, (32, 0, 4)[(j + C // 512) % 3]))
    for off in (0, 4, 32):                                              # the offset table: same shape, each offset, both input types
        out.append((2, 33 * 256 + 7, 128, 1, 0, 1e-6, 256, off))
        out.append((1, 9 * 256 + 131, 512, 0, 1, 1e-5, 256, off))
    return out


CASES = _cases()
CPU_CASES = [c for c in CASES if min(max(c[1] // 256, 1), c[6]) <= 300]


def _id(c):
    N, HW, C, f32, silu, eps, ms, off = c
    return f"N{N}-HW{HW}-C{C}-{'f32' if f32 else 'f16'}-silu{silu}-eps{eps:g}-ms{ms}-off{off}"


def n_slabs(HW, max_slabs):
    return min(max(HW // 256, 1), max_slabs)


def chain_len(HW, C, slabs):
    per = -(-HW // slabs)
    px = 2048 // C
    return 1 + 2 * (-(-per // px)) + px + C // 128


def gn_inputs(case, dev):
    """-> x [N, HW, C] (fp32 or f16), gamma, beta [C] fp32.  eps = 1e-5 cases: group 5 has variance 1e-5."""
    N, HW, C, f32, silu, eps, ms, off = case
    g = torch.Generator(dev).manual_seed(HW * 7 + C + off)
    cpg = C // 32
    sigma = 2.0 ** (torch.rand(N, 1, 32, 1, generator=g, device=dev) * 4 - 2)
    if eps == 1e-5:
        sigma[:, :, 5] = math.sqrt(1e-5)
    sign = torch.where(torch.rand(N, 1, 32, 1, generator=g, device=dev) < 0.5, -1.0, 1.0)
    x = torch.randn(N, HW, 32, cpg, generator=g, device=dev)
    x.mul_(sigma).add_(sign * off * sigma)
    x = x.view(N, HW, C)
    gamma, beta = torch.randn(C, generator=g, device=dev), torch.randn(C, generator=g, device=dev)
    return (x if f32 else x.half()), gamma, beta


# ------------------------------------------------------------------------------------------------ fp64 references and bounds
def stats_ref(x, C, eps, slabs):
    """-> (mean, rstd, bound_mean, bound_rstd), fp64 [N, 32] (module docstring)."""
    N, HW, _ = x.shape
    xd = x.double().view(N, HW, 32, C // 32)
    count = HW * (C // 32)
    mean = xd.sum((1, 3)) / count
    s1 = xd.abs().sum((1, 3)) / count
    e2 = (xd * xd).sum((1, 3)) / count
    var = ((xd - mean.view(N, 1, 32, 1)) ** 2).sum((1, 3)) / count
    rstd = 1.0 / torch.sqrt(var + _f32(eps))
    n = chain_len(HW, C, slabs)
    dm = n * U32 * s1
    dvar = (n + 1) * U32 * e2 + 2 * mean.abs() * dm + dm * dm
    return mean, rstd, dm + U32 * mean.abs(), 0.5 * rstd ** 3 * dvar + U32 * rstd


def _per_channel(v, C):
    """[N, 32] -> [N, 1, C]"""
    return v.repeat_interleave(C // 32, dim=1).unsqueeze(1)


def apply_ref(x, mean, rstd, gamma, beta, silu):
    """-> (want, dt): fp64 (x - mean) rstd gamma + beta [SiLU] on the given statistics [N, 32] and the bound of the fp32 chain."""
    C = x.shape[2]
    prod = (x.double() - _per_channel(mean.double(), C)) * _per_channel(rstd.double(), C) * gamma.double()
    t = prod + beta.double()
    dt = 4 * U32 * (prod.abs() + beta.double().abs())
    if not silu:
        return t, dt
    want = t * torch.sigmoid(t)
    return want, 1.1 * dt + U32 * (4 + 2 * t.abs() * torch.sigmoid(-t)) * want.abs()


def y_bound(want, dt):
    return dt * (1 + U16) + torch.clamp(U16 * want.abs(), min=SUB16)


def sum_bound(want, dt):
    return dt + torch.clamp(2.0 ** -22 * want.abs(), min=SUB16 / 2)


def f16_ulp(v):
    return torch.clamp(2.0 ** (torch.floor(torch.log2(v.abs().clamp(min=1e-30))) - 10), min=SUB16)


# ------------------------------------------------------------------------------------------------ the kernels restated in fp32
STAT_MUTANTS = ("finalize_tail_dropped", "eps_1e-6")
APPLY_MUTANTS = ("g1_is_g0",)


def stats_f32(x, C, eps, slabs, mutant=None):
    """gn_partial_kernel's summation tree in torch fp32 (one rounding per operation, the kernel's order) + the fp64 finalize -> fp32 [N, 32, 2]."""
    N, HW, _ = x.shape
    per = -(-HW // slabs)
    px = 2048 // C
    it = -(-per // px)
    xf = x.float()
    xf = torch.nn.functional.pad(xf, (0, 0, 0, slabs * per - HW)).view(N, slabs, per, C)      # zeros add exactly nothing
    xf = torch.nn.functional.pad(xf, (0, 0, 0, it * px - per)).view(N, slabs, it, px, C // 4, 4)
    s = torch.zeros(N, slabs, px, C // 4, device=x.device)
    q = torch.zeros_like(s)
    for i in range(it):
        f = xf[:, :, i]
        for a in (0, 2):
            s = s + (f[..., a] + f[..., a + 1])
            q = q + (f[..., a] * f[..., a] + f[..., a + 1] * f[..., a + 1])
    cs, cq = torch.zeros_like(s[:, :, 0]), torch.zeros_like(s[:, :, 0])
    for lane in range(px):
        cs, cq = cs + s[:, :, lane], cq + q[:, :, lane]
    cpc = C // 128
    cs, cq = cs.view(N, slabs, 32, cpc), cq.view(N, slabs, 32, cpc)
    gs, gq = torch.zeros_like(cs[..., 0]), torch.zeros_like(cs[..., 0])
    for k in range(cpc):
        gs, gq = gs + cs[..., k], gq + cq[..., k]
    if mutant == "finalize_tail_dropped":     # only the slabs the four-chain loop reaches: k with 32 (k / 32) + k % 8 + 24 < slabs
        k = torch.arange(slabs, device=x.device)
        keep = (32 * (k // 32) + k % 8 + 24 < slabs).view(1, slabs, 1)
        gs, gq = gs * keep, gq * keep
    count = float(np.float32(HW) * np.float32(C // 32))
    mean = gs.double().sum(1) / count
    var = torch.clamp(gq.double().sum(1) / count - mean * mean, min=0.0)
    rstd = 1.0 / torch.sqrt(var + _f32(1e-6 if mutant == "eps_1e-6" else eps))
    return torch.stack([mean.float(), rstd.float()], dim=2)


def _fma(a, b, c):
    """fp32 fused multiply-add: the product of two floats is exact in fp64, the sum is rounded there and again to fp32"""
    return (a.double() * b.double() + c.double()).float()


def apply_f32(x, stats, gamma, beta, silu, mutant=None):
    """gn_apply_kernel in torch fp32 -> (o fp32, y f16, y_lo f16)"""
    C = x.shape[2]
    mean, rstd = stats[..., 0], stats[..., 1]
    if mutant == "g1_is_g0":       # the octet's second half read with the first half's group
        cpg = C // 32
        g0 = (torch.arange(C, device=x.device) // 8 * 8) // cpg
        m, r = mean[:, g0].unsqueeze(1), rstd[:, g0].unsqueeze(1)
    else:
        m, r = _per_channel(mean, C), _per_channel(rstd, C)
    a = (x.float() - m) * r
    o = _fma(a, gamma, beta)
    if silu:
        o = o / (1.0 + torch.exp(-o))
    y = o.half()
    return o, y, (o - y.float()).half()


# ------------------------------------------------------------------------------------------------ the checks, shared by both halves
def _worst(tag, got, want, bound):
    err = (got.double() - want).abs()
    bad = ~(err <= bound)
    ratio = float((err / bound).max())
    if bool(bad.any()):
        i = int(torch.nonzero(bad.reshape(-1))[0])
        raise AssertionError(f"{tag}: {int(bad.sum())} of {err.numel()} out of bound; first at {i}: got {float(got.reshape(-1)[i]):.9e} want "
                             f"{float(want.reshape(-1)[i]):.9e} err {float(err.reshape(-1)[i]):.3e} > {float(bound.reshape(-1)[i]):.3e}; worst err / bound {ratio:.3g}")
    return ratio


def check_case(tag, case, x, gamma, beta, stats, y, y_lo):
    """stats fp32 [N, 32, 2], y / y_lo f16 [N, HW, C] as produced for `case` -> dict of worst err / bound.  Raises on a miss."""
    N, HW, C, f32, silu, eps, ms, off = case
    slabs = n_slabs(HW, ms)
    mean, rstd, bm, br = stats_ref(x, C, eps, slabs)
    res = {"mean": _worst(tag + " mean", stats[..., 0], mean, bm), "rstd": _worst(tag + " rstd", stats[..., 1], rstd, br)}
    want, dt = apply_ref(x, stats[..., 0], stats[..., 1], gamma, beta, silu)
    res["y"] = _worst(tag + " y", y, want, y_bound(want, dt))
    res["y+y_lo"] = _worst(tag + " y + y_lo", y.double() + y_lo.double(), want, sum_bound(want, dt))
    if not silu:
        o, yr, lor = apply_f32(x, stats, gamma, beta, 0)
        clear = yr.view(torch.int16) == y.view(torch.int16)
        res["lo_skipped"] = 1.0 - float(clear.double().mean())
        assert res["lo_skipped"] <= 0.01, f"{tag}: o ambiguous at {res['lo_skipped']:.3%} of the elements"
        same = (lor.view(torch.int16) == y_lo.view(torch.int16)) | ~clear
        assert bool(same.all()), f"{tag}: y_lo != f16(o - y) at {int((~same).sum())} elements"
    true_want, _ = apply_ref(x, mean, rstd, gamma, beta, silu)
    dev_true = (y.double() - true_want).abs()
    res["ulps_vs_true"] = float((dev_true / f16_ulp(true_want)).max())      # in ulps of the element itself: near-zero outputs dominate
    res["abs_vs_true"] = float(dev_true.max()) / 2.0 ** -10                   # in ulps of an output of magnitude 1
    return res


def _report(tag, res):
    print(f"groupnorm {tag}: err / bound " + " ".join(f"{k} {v:.3g}" for k, v in res.items() if k not in ("lo_skipped", "ulps_vs_true", "abs_vs_true")) +
          f" | y vs true GroupNorm {res['ulps_vs_true']:.2f} f16 ulps of the element, {res['abs_vs_true']:.3f} ulps of 1.0" + (f" | y_lo skipped {res['lo_skipped']:.2%}" if "lo_skipped" in res else ""))


# ------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("case", CPU_CASES, ids=_id)
def test_restatement_within_bounds(case):
    """the fp32 restatement of the three kernels, rounding where they round, passes every check the GPU result has to pass"""
    N, HW, C, f32, silu, eps, ms, off = case
    x, gamma, beta = gn_inputs(case, torch.device("cpu"))
    stats = stats_f32(x, C, eps, n_slabs(HW, ms))
    _, y, y_lo = apply_f32(x, stats, gamma, beta, silu)
    res = check_case(_id(case), case, x, gamma, beta, stats, y, y_lo)
    assert max(res["mean"], res["rstd"], res["y"], res["y+y_lo"]) < 1.0
    _report(_id(case), res)


def test_named_mistakes_leave_the_bounds():
    """finalize without its tail loop (33 slabs: slab 32 is lost; 9 slabs: everything), eps 1e-6 where 1e-5 was asked for (group 5 has
    variance 1e-5), gn_apply's second half octet read with g0 (C = 128 only: an octet spans two groups there)."""
    dev = torch.device("cpu")
    for case, mutant in [((2, 33 * 256 + 7, 128, 1, 0, 1e-6, 256, 0), "finalize_tail_dropped"), ((3, 9 * 256 + 255, 128, 1, 0, 1e-5, 256, 4), "finalize_tail_dropped"),
                         ((1, 9 * 256 + 131, 512, 0, 1, 1e-5, 256, 0), "eps_1e-6"), ((1, 25 * 256, 128, 1, 0, 1e-5, 256, 32), "eps_1e-6")]:
        N, HW, C, f32, silu, eps, ms, off = case
        x, gamma, beta = gn_inputs(case, dev)
        slabs = n_slabs(HW, ms)
        mean, rstd, bm, br = stats_ref(x, C, eps, slabs)
        good, bad = stats_f32(x, C, eps, slabs), stats_f32(x, C, eps, slabs, mutant)
        assert bool(((good[..., 1].double() - rstd).abs() <= br).all())
        worst = float(((bad[..., 1].double() - rstd).abs() / br).max())
        print(f"{mutant} on {_id(case)}: rstd err / bound {worst:.3g}")
        assert worst > 10.0, (mutant, _id(case), worst)
    case = (2, 2 * 256, 128, 0, 1, 1e-6, 256, 4)
    x, gamma, beta = gn_inputs(case, dev)
    stats = stats_f32(x, 128, 1e-6, 2)
    want, dt = apply_ref(x, stats[..., 0], stats[..., 1], gamma, beta, 1)
    _, y, _ = apply_f32(x, stats, gamma, beta, 1, "g1_is_g0")
    worst = float(((y.double() - want).abs() / y_bound(want, dt)).max())
    print(f"g1_is_g0 on {_id(case)}: y err / bound {worst:.3g}")
    assert worst > 10.0
    for C in (256, 512):    # and no difference at the wider maps: the mistake can show at C = 128 only
        xs = torch.randn(1, 256, C)
        st = stats_f32(xs, C, 1e-6, 1)
        g, b = torch.randn(C), torch.randn(C)
        assert torch.equal(apply_f32(xs, st, g, b, 0)[1], apply_f32(xs, st, g, b, 0, "g1_is_g0")[1])


def test_emulated_fma_is_rarely_double_rounded():
    """y_lo's equality check skips elements whose restated o does not round to the stored y; the restatement's own ambiguity -- the fp64 sum
    of _fma rounded twice -- must stay far below the 1 % allowed"""
    g = torch.Generator().manual_seed(1)
    a, b, c = (torch.randn(1 << 20, generator=g) for _ in range(3))
    exact = torch.from_numpy((a.numpy().astype(np.longdouble) * b.numpy().astype(np.longdouble) + c.numpy().astype(np.longdouble)).astype(np.float32))
    assert float((exact != _fma(a, b, c)).double().mean()) < 1e-4


def test_hook_refuses_what_its_comment_says(lib):
    """argument checks come before any device work, so they run without a GPU"""
    import ctypes
    buf = torch.zeros(4096)
    p = ctypes.c_void_p(buf.data_ptr())
    assert buf.data_ptr() % 16 == 0
    null = ctypes.c_void_p(None)

    def rc(N=1, HW=256, C=128, eps=1e-6, ms=256, dt=1, x=p, y=p):
        return lib.latte_debug_groupnorm_ex(x, 1, y, null, p, p, N, HW, C, 0, eps, ms, null, dt, null)
    assert rc(ms=0) == LATTE_ERR_INVALID and b"max_slabs" in lib.latte_last_error()
    assert rc(N=2, ms=257) == LATTE_ERR_INVALID and b"max_slabs" in lib.latte_last_error()
    assert rc(N=1, ms=256 * 64 + 1) == LATTE_ERR_INVALID and b"max_slabs" in lib.latte_last_error()
    assert rc(C=64) == LATTE_ERR_INVALID and b"C must be" in lib.latte_last_error()
    assert rc(dt=0) == LATTE_ERR_INVALID and b"f16" in lib.latte_last_error()
    assert rc(x=null) == LATTE_ERR_INVALID
    assert rc(y=ctypes.c_void_p(buf.data_ptr() + 8)) == LATTE_ERR_INVALID
    assert rc(eps=0.0) == LATTE_ERR_INVALID


# ------------------------------------------------------------------------------------------------ GPU
def _guarded_half(N, HW, C, dev):
    buf = torch.full(((N * HW + 2 * GUARD) * C,), SENT, dtype=torch.float16, device=dev)
    view = buf[GUARD * C:(GUARD + N * HW) * C].view(N, HW, C)
    view.fill_(float("nan"))
    return buf, view


def _guards_intact(tag, buf, view):
    assert not bool(torch.isnan(view).any()), f"{tag}: elements left unwritten"
    view.fill_(SENT)
    assert bool((buf == SENT).all()), f"{tag}: wrote outside its range"


@gpu
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_groupnorm_ex(lib, case):
    from latte_amd._lib import check, ptr, stream_ptr
    N, HW, C, f32, silu, eps, ms, off = case
    dev = torch.device("cuda")
    x, gamma, beta = gn_inputs(case, dev)
    stats = torch.full((N, 32, 2), float("nan"), device=dev)
    ybuf, y = _guarded_half(N, HW, C, dev)
    check(lib.latte_debug_groupnorm_ex(ptr(x), f32, ptr(y), None, ptr(gamma), ptr(beta), N, HW, C, silu, eps, ms, ptr(stats), 1, stream_ptr()))
    torch.cuda.synchronize()
    y_alone, stats_alone = y.clone(), stats.clone()
    _guards_intact(_id(case) + " y", ybuf, y)
    y.fill_(float("nan"))
    lbuf, y_lo = _guarded_half(N, HW, C, dev)
    check(lib.latte_debug_groupnorm_ex(ptr(x), f32, ptr(y), ptr(y_lo), ptr(gamma), ptr(beta), N, HW, C, silu, eps, ms, ptr(stats), 1, stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(y.view(torch.int16), y_alone.view(torch.int16)), "y changes when y_lo is asked for"
    assert torch.equal(stats, stats_alone)
    res = check_case(_id(case), case, x, gamma, beta, stats, y, y_lo.clone())
    _report(_id(case), res)
    _guards_intact(_id(case) + " y (split)", ybuf, y)
    _guards_intact(_id(case) + " y_lo", lbuf, y_lo)
