"""The VAE decoder's small kernels (csrc/vae.hip) and convert_split (csrc/pointwise.hip), one launcher at a time through the
latte_debug_vae_* hooks, per element against fp64.  Every output is NaN before the launch and lies between sentinel guards that must come
back untouched.  u = 2^-24; all half buffers are f16.

Bounds.  A sum b + sum_i a_i w_i formed in fp32 is off by at most u times the sum of the magnitudes of its rounded intermediate results
(every operation rounds once, relative to its own result); each partial sum is at most |b| + sum |a_i| |w_i|, so a chain of n roundings
gives the gamma_n form  n u (|b| + sum_i |a_i| |w_i|).  n per kernel, counting the longest path an addend takes:

  post_quant      z z_scale (1), the product with w (1), four additions (4): n = 6.  The kernel carries no contract pragma; a fused
                  multiply-add drops the product's rounding, so 6 covers both forms.
  conv_in         a0 = fmaf(patch[k], w, a0) from the bias over 36 taps, and the bias itself: n = 37.
  conv_out        conv_out_kernel: one thread per pixel, fmaf over 9 C products from the bias.  conv_out_c128_kernel (C == 128 and
                  W % 16 == 0): 16 lanes per pixel, 72 products each from zero, four xor-shuffle additions, then the bias.  With x_lo
                  the operand is fp32(hi) + fp32(lo): one more rounding per product.  Both forms are held to the sharper, running-sum
                  statement of the same bound, u (sum over the kernel's own intermediate sums |s_k|  +  sum |a_i w_i| for the hi + lo
                  addition), with the s_k taken from the fp64 terms in the kernel's order: generic (bias, tap-major, channels) and
                  c128 (per lane tap-major over its 8 channels, the shuffle tree, the bias).  It is never above n u (|b| + sum |a_i|
                  |w_i|) with n = 9 C + 2 (generic) and 78 (c128), which is asserted alongside; only the sharper form can tell a run
                  that ignores x_lo from one that does not at C = 512, where 9 C u is already 2^-12.  The x_lo inputs are true f16
                  rounding residuals of an fp32 tensor whose residual has the sign of the channel's weights, so that dropping x_lo
                  moves every output the same way (asserted on the CPU: more than 10 x the bound).
                  out_mode 1 must equal sample.py:122 evaluated in torch fp32 on the same inputs' out_mode 0 result, exactly.
  time_conv_out   o += w v over 3 taps x 3 channels from the bias: n = 10.  out_mode 1: with the identity on the centre tap and bias 0
                  the fp32 value is the input exactly; 2^22 inputs, among them every level boundary ((m - 1/2) / 255 2 - 1 and k / 255
                  2 - 1) and the 4 fp32 neighbours on either side of each, must give the bytes of the torch fp32 formula.
  softmax_rows    a_c = s_c scale (u |a_c|), the maximum m carries the same rounding (u |m|), d_c = a_c - m (u |d_c|; fused with the
                  product: the same three terms bound it): the argument is off by dz_c = u (|a_c| + |m| + |d_c|).  __expf(d) multiplies
                  by log2(e) (constant and product: 2 u |d| in the result) and takes v_exp_f32 (one ulp = 2 u): e_c is off by the factor
                  rho_c = dz_c + (2 |d_c| + 2) u.  The row sum adds L / 64 terms per lane and six shuffle stages: (L / 64 + 6) u, and
                  carries sum_k P_k rho_k; the reciprocal and the product add u each.  p is then rounded to f16:
                  |dp| <= P_c (rho_c + sum_k P_k rho_k + (L / 64 + 8) u) (1 + 2^-11) + max(2^-11 P_c, 2^-24),
                  the floor being the spacing of the f16 subnormals.  Rows: N(0, 30^2) scores, an all-equal row, a row with a spike of
                  +2000 in the last column (overflows without the max subtraction).
  pack_conv_w, pack_conv_t (no mix), convert_split
                  pure layout + rounding: bit for bit against torch (permute, .half(), (v - v.half().float()).half()), Cout != Cin so a
                  swapped index shows, inputs reaching into the f16 subnormal range.
  pack_conv_t with mix, scale_by_sigmoid
                  sc = 1 / (1 + __expf(-mix)): the exponential is off by (2 |mix| + 2) u, scaled by sigmoid(-mix) <= 1 in the sum,
                  the sum and the division add u each, the product with w one more: tau = (5 + 2 |mix|) u relative.
                  scale_by_sigmoid: |out - in sigma| <= tau |in sigma|.  pack_conv_t: hi + lo recovers the fp32 product up to the
                  f16 rounding of the residual, 2^-22 |w sigma| while the residual is a normal f16 number; packed weights are small
                  (|w| ~ (3 Cin)^-1/2), their residuals lie among the f16 subnormals, where the rounding error is 2^-25 whatever |w|:
                  |hi + lo - w sigma| <= max(2^-22 |w sigma|, 2^-25) + tau |w sigma|.

The CPU half (not marked gpu) restates every kernel in torch fp32, rounding where the kernel rounds, runs it through the same checks on
the same cases, and shows that each of these mistakes leaves the bounds: conv_out without x_lo, a border tap clamped instead of
skipped, softmax without the max subtraction, time_conv_out reading frame -1 as frame 0, pack_conv_t with tap and ci swapped, z_scale
applied after the bias.

Worst err / bound per kernel is printed by every test; the MI355X figures are in DESIGN.md section 4.8."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

from test_vae_groupnorm import LATTE_ERR_INVALID, SUB16, U16, U32, _fma, _worst

gpu = pytest.mark.gpu
SENT = -7.25
PAD = 64
CPU = torch.device("cpu")


def _gen(seed, dev):
    return torch.Generator(dev).manual_seed(seed)


def _guarded(n, dtype, dev):
    """-> (buf, view): n elements of NaN (0xFF bytes for uint8) between PAD sentinel elements"""
    sent = 0xA5 if dtype == torch.uint8 else SENT
    buf = torch.full((PAD + n + PAD,), sent, dtype=dtype, device=dev)
    view = buf[PAD:PAD + n]
    view.fill_(0xFF if dtype == torch.uint8 else float("nan"))
    return buf, view


def _guards_intact(tag, buf, view):
    """after the last read of `view` (it is overwritten)"""
    sent = 0xA5 if buf.dtype == torch.uint8 else SENT
    if buf.dtype != torch.uint8:
        assert not bool(torch.isnan(view).any()), f"{tag}: elements left unwritten"
    view.fill_(sent)
    assert bool((buf == sent).all()), f"{tag}: wrote outside its range"


def _call(lib, name, *args):
    from latte_amd._lib import check, ptr, stream_ptr
    check(getattr(lib, name)(*[ptr(a) if (a is None or torch.is_tensor(a)) else a for a in args], stream_ptr()))
    torch.cuda.synchronize()


def to_uint8(v):
    """sample.py:122 in torch fp32, one rounding per operation"""
    return ((v * 0.5 + 0.5) * 255.0 + 0.5).clamp(0.0, 255.0).to(torch.uint8)


# ================================================================================================ post_quant
PQ_CASES = [(3, 7, 1.0), (2, 256, 1.0), (3, 7, 1.0 / 0.18215), (2, 256, 1.0 / 0.18215)]


def pq_inputs(case, dev):
    N, hw, zs = case
    g = _gen(N * 100 + hw, dev)
    return torch.randn(N, 4, hw, generator=g, device=dev), torch.randn(4, 4, generator=g, device=dev), torch.randn(4, generator=g, device=dev)


def pq_ref(z, w, b, zs):
    """-> (want, bound) fp64 [N, hw, 4]"""
    zs = float(torch.tensor(zs, dtype=torch.float32))
    v = z.double().permute(0, 2, 1) * zs
    want = v @ w.double().t() + b.double()
    return want, 6 * U32 * (v.abs() @ w.double().abs().t() + b.double().abs())


def pq_f32(z, w, b, zs, mutant=None):
    zs = torch.tensor(zs, dtype=torch.float32, device=z.device)
    v = z.permute(0, 2, 1) * (1.0 if mutant == "scale_after_bias" else zs)
    o = b.expand(v.shape[0], v.shape[1], 4).clone()
    for c in range(4):
        o = o + w[:, c] * v[..., c:c + 1]
    return o * zs if mutant == "scale_after_bias" else o


@pytest.mark.parametrize("case", PQ_CASES, ids=str)
def test_post_quant_restated(case):
    z, w, b = pq_inputs(case, CPU)
    want, bound = pq_ref(z, w, b, case[2])
    print("post_quant restated: err / bound", _worst("post_quant", pq_f32(z, w, b, case[2]), want, bound))
    bad = (pq_f32(z, w, b, case[2], "scale_after_bias").double() - want).abs() / bound
    assert case[2] == 1.0 or float(bad.max()) > 10.0


@gpu
@pytest.mark.parametrize("case", PQ_CASES, ids=str)
def test_post_quant(lib, case):
    dev = torch.device("cuda")
    N, hw, zs = case
    z, w, b = pq_inputs(case, dev)
    buf, out = _guarded(N * hw * 4, torch.float32, dev)
    _call(lib, "latte_debug_vae_post_quant", z, w, b, out, N, hw, zs)
    want, bound = pq_ref(z, w, b, zs)
    print(f"post_quant {case}: err / bound {_worst('post_quant', out.view(N, hw, 4), want, bound):.3g}")
    _guards_intact("post_quant", buf, out)


# ================================================================================================ conv_in
CI_CASES = [(2, 3, 5, 512), (1, 1, 1, 128), (1, 4, 4, 1024)]


def ci_inputs(case, dev):
    N, H, W, Cout = case
    g = _gen(H * 10 + W + Cout, dev)
    return (torch.randn(N, H, W, 4, generator=g, device=dev), torch.randn(Cout, 4, 3, 3, generator=g, device=dev) / 6.0,
            torch.randn(Cout, generator=g, device=dev))


def ci_ref(x, w, b):
    """-> (want, bound) fp64 NHWC"""
    xd, wd, bd = x.double().permute(0, 3, 1, 2), w.double(), b.double()
    want = F.conv2d(xd, wd, bd, padding=1)
    mag = F.conv2d(xd.abs(), wd.abs(), bd.abs(), padding=1)
    return want.permute(0, 2, 3, 1), 37 * U32 * mag.permute(0, 2, 3, 1)


def _patches(x, clamp=False):
    """x NHWC [N, H, W, C] -> [N, H, W, 9, C]: tap (ky, kx) of every pixel, zero outside (clamp: the nearest pixel instead, the mistake)"""
    xp = F.pad(x.permute(0, 3, 1, 2), (1, 1, 1, 1), mode="replicate" if clamp else "constant").permute(0, 2, 3, 1)
    H, W = x.shape[1], x.shape[2]
    return torch.stack([xp[:, ky:ky + H, kx:kx + W] for ky in range(3) for kx in range(3)], dim=3)


def ci_f32(x, w, b, clamp=False):
    N, H, W, _ = x.shape
    p = _patches(x, clamp).reshape(N, H, W, 36)                 # k = tap 4 + ci
    wt = w.permute(2, 3, 1, 0).reshape(36, -1)                  # [k][co]
    a = b.expand(N, H, W, -1).clone()
    for k in range(36):
        a = _fma(p[..., k:k + 1], wt[k], a)
    return a


@pytest.mark.parametrize("case", CI_CASES, ids=str)
def test_conv_in_restated(case):
    x, w, b = ci_inputs(case, CPU)
    want, bound = ci_ref(x, w, b)
    print("conv_in restated: err / bound", _worst("conv_in", ci_f32(x, w, b), want, bound))
    if case[1] > 1:
        assert float(((ci_f32(x, w, b, clamp=True).double() - want).abs() / bound).max()) > 10.0


@gpu
@pytest.mark.parametrize("case", CI_CASES, ids=str)
def test_conv_in(lib, case):
    dev = torch.device("cuda")
    N, H, W, Cout = case
    x, w, b = ci_inputs(case, dev)
    buf, out = _guarded(N * H * W * Cout, torch.float32, dev)
    _call(lib, "latte_debug_vae_conv_in", x, w, b, out, N, H, W, Cout)
    want, bound = ci_ref(x, w, b)
    print(f"conv_in {case}: err / bound {_worst('conv_in', out.view(N, H, W, Cout), want, bound):.3g}")
    _guards_intact("conv_in", buf, out)


# ================================================================================================ conv_out
CO_CASES = [(2, 3, 16, 128), (1, 1, 32, 128), (3, 2, 48, 128),          # conv_out_c128_kernel
            (1, 5, 24, 128), (2, 3, 16, 256), (1, 2, 8, 512)]           # conv_out_kernel


def is_c128(case):
    return case[3] == 128 and case[2] % 16 == 0


def co_inputs(case, dev):
    """-> hi, lo f16 NHWC, w fp32 [3, C, 3, 3], b [3].  hi + lo are the f16 split of an fp32 tensor whose rounding residual has the sign
    of its channel's weights (0.45 f16 ulps of magnitude); weights and bias are scaled so that the outputs span [-1.5, 1.5]."""
    N, H, W, C = case
    g = _gen(H * 100 + W + C, dev)
    wsign = torch.where(torch.rand(C, generator=g, device=dev) < 0.5, -1.0, 1.0)
    w = torch.rand(3, C, 3, 3, generator=g, device=dev) * wsign.view(1, C, 1, 1)
    h = torch.randn(N, H, W, C, generator=g, device=dev).half().float()
    ulp = 2.0 ** (torch.floor(torch.log2(h.abs().clamp(min=2.0 ** -14))) - 10)
    x32 = h + 0.45 * ulp * wsign
    hi = x32.half()
    raw = F.conv2d(hi.double().permute(0, 3, 1, 2), w.double(), padding=1)      # scale and centre: the outputs span [-1.5, 1.5]
    k = 3.0 / float(raw.max() - raw.min())
    b = torch.full((3,), -0.5 * k * float(raw.max() + raw.min()), device=dev) + torch.tensor([0.0, 1e-3, -1e-3], device=dev)
    return hi, (x32 - hi.float()).half(), w * k, b


def co_ref(case, hi, lo, w, b):
    """-> (want, bound, loose) fp64 [N, 3, H, W] (module docstring); lo may be None"""
    N, H, W, C = case
    f = hi.double() + (lo.double() if lo is not None else 0.0)
    terms = _patches(f).unsqueeze(3) * w.double().permute(0, 2, 3, 1).reshape(3, 9, C)          # [N, H, W, 3, 9, C]
    mag = terms.abs().sum((4, 5))
    bd = b.double().view(3)
    split = mag if lo is not None else 0.0
    if is_c128(case):
        lane = terms.view(N, H, W, 3, 9, 16, 8).permute(0, 1, 2, 3, 5, 4, 6).reshape(N, H, W, 3, 16, 72).cumsum(-1)
        inter = lane.abs().sum((4, 5))
        node = lane[..., -1]
        for _ in range(4):
            node = node[..., 0::2] + node[..., 1::2]
            inter = inter + node.abs().sum(-1)
        want = node[..., 0] + bd
        n = 78
    else:
        s = bd.view(3, 1) + terms.reshape(N, H, W, 3, 9 * C).cumsum(-1)
        inter = s.abs().sum(-1)
        want = s[..., -1]
        n = 9 * C + 2
    bound = U32 * (inter + want.abs() + split) * (1 + 1e-3)
    loose = n * U32 * (mag + bd.abs())
    assert bool((bound <= loose).all())
    return want.permute(0, 3, 1, 2), bound.permute(0, 3, 1, 2), loose.permute(0, 3, 1, 2)


def co_f32(case, hi, lo, w, b, clamp=False):
    """both kernels in torch fp32 -> [N, 3, H, W]"""
    N, H, W, C = case
    f = hi.float() + lo.float() if lo is not None else hi.float()
    p = _patches(f, clamp)                                                                        # [N, H, W, 9, C]
    wt = w.permute(0, 2, 3, 1).reshape(3, 9, C)
    if is_c128(case):
        pl = p.view(N, H, W, 1, 9, 16, 8)
        wl = wt.view(3, 9, 16, 8)
        acc = torch.zeros(N, H, W, 3, 16, device=hi.device)
        for tap in range(9):
            for e in range(8):
                acc = _fma(pl[..., tap, :, e], wl[:, tap, :, e], acc)
        for _ in range(4):
            acc = acc[..., 0::2] + acc[..., 1::2]
        out = acc[..., 0] + b
    else:
        out = b.expand(N, H, W, 3).clone()
        pf, wf = p.reshape(N, H, W, 1, 9 * C), wt.reshape(3, 9 * C)
        for k in range(9 * C):
            out = _fma(pf[..., k], wf[:, k], out)
    return out.permute(0, 3, 1, 2)


@pytest.mark.parametrize("case", CO_CASES, ids=str)
def test_conv_out_restated(case):
    hi, lo, w, b = co_inputs(case, CPU)
    for l in (None, lo):
        want, bound, loose = co_ref(case, hi, l, w, b)
        got = co_f32(case, hi, l, w, b)
        print(f"conv_out restated {case} lo={l is not None}: err / bound {_worst('conv_out', got, want, bound):.3g}, outputs in "
              f"[{float(want.min()):.2f}, {float(want.max()):.2f}]")
        assert float(want.min()) < -1.0 and float(want.max()) > 1.0             # both clamps of out_mode 1 are reached
    ignored = ((co_f32(case, hi, None, w, b).double() - want).abs() / bound)     # x_lo dropped, against the split reference
    print(f"conv_out {case} without x_lo: err / bound min {float(ignored.min()):.3g} median {float(ignored.median()):.3g}")
    assert float(ignored.median()) > 10.0
    if case[1] > 1:
        assert float(((co_f32(case, hi, lo, w, b, clamp=True).double() - want).abs() / bound).max()) > 10.0


@gpu
@pytest.mark.parametrize("case", CO_CASES, ids=str)
def test_conv_out(lib, case):
    dev = torch.device("cuda")
    N, H, W, C = case
    hi, lo, w, b = co_inputs(case, dev)
    for l in (None, lo):
        buf, out = _guarded(N * 3 * H * W, torch.float32, dev)
        _call(lib, "latte_debug_vae_conv_out", hi, l, w, b, out, N, H, W, C, 0)
        want, bound, _ = co_ref(case, hi, l, w, b)
        got = out.view(N, 3, H, W).clone()
        print(f"conv_out {'c128' if is_c128(case) else 'generic'} {case} lo={l is not None}: err / bound {_worst('conv_out', got, want, bound):.3g}")
        _guards_intact("conv_out", buf, out)
        b8, o8 = _guarded(N * H * W * 3, torch.uint8, dev)
        _call(lib, "latte_debug_vae_conv_out", hi, l, w, b, o8, N, H, W, C, 1)
        ref8 = to_uint8(got.cpu()).permute(0, 2, 3, 1)
        assert int(ref8.min()) == 0 and int(ref8.max()) == 255
        assert torch.equal(o8.view(N, H, W, 3).cpu(), ref8), "uint8 output differs from sample.py:122 on the fp32 output"
        _guards_intact("conv_out uint8", b8, o8)


# ================================================================================================ softmax_rows
SM_ROWS, SM_L, SM_SCALES = (1, 5, 7, 8), (64, 192, 256, 4096), (512 ** -0.5, 1.0)


def sm_inputs(rows, L, dev):
    s = torch.randn(rows, L, generator=_gen(rows * 7 + L, dev), device=dev) * 30.0
    for r in range(rows):
        if r % 4 == 1:
            s[r] = 11.5
        elif r % 4 == 2:
            s[r, L - 1] += 2000.0
    return s


def sm_ref(s, scale):
    L = s.shape[1]
    sc = float(torch.tensor(scale, dtype=torch.float32))
    a = s.double() * sc
    m = a.max(1, keepdim=True).values
    d = a - m
    P = torch.softmax(a, dim=1)
    rho = U32 * (a.abs() + m.abs() + d.abs()) + (2 * d.abs() + 2) * U32
    rel = rho + (P * rho).sum(1, keepdim=True) + (L // 64 + 8) * U32
    return P, P * rel * (1 + U16) + torch.clamp(U16 * P, min=SUB16)


def sm_f32(s, scale, no_max=False):
    L = s.shape[1]
    a = s * torch.tensor(scale, dtype=torch.float32, device=s.device)
    m = torch.zeros_like(a[:, :1]) if no_max else a.max(1, keepdim=True).values
    e = torch.exp(a - m)
    lanes = e.view(-1, L // 64, 64)
    tot = torch.zeros_like(lanes[:, 0])
    for j in range(L // 64):
        tot = tot + lanes[:, j]
    for _ in range(6):
        tot = tot[:, 0::2] + tot[:, 1::2]
    return (e * (1.0 / tot)).half()


@pytest.mark.parametrize("L", SM_L)
def test_softmax_rows_restated(L):
    worst = 0.0
    for rows in SM_ROWS:
        for scale in SM_SCALES:
            s = sm_inputs(rows, L, CPU)
            want, bound = sm_ref(s, scale)
            worst = max(worst, _worst(f"softmax rows {rows} L {L} scale {scale:.3g}", sm_f32(s, scale), want, bound))
            if rows >= 3 and scale == 1.0:     # the spike row: exp(2000) overflows
                assert not bool(((sm_f32(s, scale, no_max=True).double() - want).abs() <= bound).all())
    print(f"softmax_rows restated L {L}: err / bound {worst:.3g}")


@gpu
@pytest.mark.parametrize("L", SM_L)
def test_softmax_rows(lib, L):
    dev = torch.device("cuda")
    worst, flushed = 0.0, 0
    for rows in SM_ROWS:
        for scale in SM_SCALES:
            s = sm_inputs(rows, L, dev)
            buf, p = _guarded(rows * L, torch.float16, dev)
            _call(lib, "latte_debug_vae_softmax_rows", s, p, rows, L, scale)
            want, bound = sm_ref(s, scale)
            got = p.view(rows, L).clone()
            flushed += int(((got == 0) & (want >= SUB16)).sum())
            worst = max(worst, _worst(f"softmax rows {rows} L {L} scale {scale:.3g}", got, want, bound))
            _guards_intact("softmax_rows", buf, p)
    print(f"softmax_rows L {L}: err / bound {worst:.3g}; results >= 2^-24 stored as zero: {flushed}")


# ================================================================================================ time_conv_out
TC_CASES = [(T, HW) for T in (1, 2, 5) for HW in (7, 1024)]


def tc_ref(x, w, b):
    """x [T, 3, HW], w [3, 3, 3] = [co][ci][tap] -> (want, bound) fp64 [T, 3, HW]"""
    xd = F.pad(x.double(), (0, 0, 0, 0, 1, 1))
    T = x.shape[0]
    want = b.double().view(1, 3, 1).expand(T, 3, x.shape[2]).clone()
    mag = want.abs()
    for tap in range(3):
        want = want + torch.einsum("oc,tcp->top", w.double()[:, :, tap], xd[tap:tap + T])
        mag = mag + torch.einsum("oc,tcp->top", w.double()[:, :, tap].abs(), xd[tap:tap + T].abs())
    return want, 10 * U32 * mag


def tc_f32(x, w, b, clamp=False):
    T = x.shape[0]
    xp = torch.cat([x[:1] if clamp else torch.zeros_like(x[:1]), x, x[-1:] if clamp else torch.zeros_like(x[:1])])
    o = b.view(1, 3, 1).expand(T, 3, x.shape[2]).clone()
    for tap in range(3):
        for ci in range(3):
            o = o + w[:, ci, tap].view(1, 3, 1) * xp[tap:tap + T, ci:ci + 1]
    return o


def tc_inputs(case, dev):
    T, HW = case
    g = _gen(T * 1000 + HW, dev)
    return torch.randn(T, 3, HW, generator=g, device=dev), torch.randn(3, 3, 3, generator=g, device=dev) * 0.4, torch.randn(3, generator=g, device=dev) * 0.3


def level_probe(n):
    """n fp32 values in about [-1.3, 1.3]: every boundary of sample.py:122's 256 levels and k / 255 2 - 1, each with its 4 fp32 neighbours on
    either side, +-1, the clamps, and uniform values for the rest"""
    k = torch.arange(0, 257, dtype=torch.float64)
    base = torch.cat([(k - 0.5) / 255 * 2 - 1, k / 255 * 2 - 1, torch.tensor([-1.5, 1.5, 0.0])]).float()
    vals = [base]
    up, dn = base.clone(), base.clone()
    for _ in range(4):
        up, dn = torch.nextafter(up, torch.tensor(4.0)), torch.nextafter(dn, torch.tensor(-4.0))
        vals += [up.clone(), dn.clone()]
    v = torch.cat(vals)
    rest = torch.rand(n - v.numel(), generator=torch.Generator().manual_seed(3)) * 2.6 - 1.3
    return torch.cat([v, rest])


@pytest.mark.parametrize("case", TC_CASES, ids=str)
def test_time_conv_out_restated(case):
    x, w, b = tc_inputs(case, CPU)
    want, bound = tc_ref(x, w, b)
    print("time_conv_out restated: err / bound", _worst("time_conv_out", tc_f32(x, w, b), want, bound))
    assert float(((tc_f32(x, w, b, clamp=True).double() - want).abs() / bound).max()) > 10.0


def test_level_probe_separates_fused_rounding():
    """the probe holds inputs at which a single mis-rounded operation of sample.py:122 changes the byte: (v 0.5 + 0.5) 255 + 0.5 in fp64
    differs from the fp32 formula's bytes somewhere on it"""
    v = level_probe(1 << 16)
    assert int(to_uint8(v).min()) == 0 and int(to_uint8(v).max()) == 255
    assert not torch.equal(to_uint8(v), to_uint8(v.double()))


@gpu
@pytest.mark.parametrize("case", TC_CASES, ids=str)
def test_time_conv_out(lib, case):
    dev = torch.device("cuda")
    T, HW = case
    x, w, b = tc_inputs(case, dev)
    buf, out = _guarded(T * 3 * HW, torch.float32, dev)
    _call(lib, "latte_debug_vae_time_conv_out", x, w, b, out, T, HW, 0)
    want, bound = tc_ref(x, w, b)
    got = out.view(T, 3, HW).clone()
    print(f"time_conv_out {case}: err / bound {_worst('time_conv_out', got, want, bound):.3g}")
    _guards_intact("time_conv_out", buf, out)
    b8, o8 = _guarded(T * HW * 3, torch.uint8, dev)                      # random weights: the bytes of the same inputs' fp32 output
    _call(lib, "latte_debug_vae_time_conv_out", x, w, b, o8, T, HW, 1)
    assert torch.equal(o8.view(T, HW, 3).cpu(), to_uint8(got.cpu()).permute(0, 2, 1))
    _guards_intact("time_conv_out uint8", b8, o8)


@gpu
def test_time_conv_out_levels(lib):
    dev = torch.device("cuda")
    T, HW = 2, 699051                                                    # 3 T HW >= 2^22
    x = level_probe(T * 3 * HW).view(T, 3, HW).to(dev)
    w = torch.zeros(3, 3, 3, device=dev)
    for c in range(3):
        w[c, c, 1] = 1.0
    b = torch.zeros(3, device=dev)
    buf, out = _guarded(T * 3 * HW, torch.float32, dev)
    _call(lib, "latte_debug_vae_time_conv_out", x, w, b, out, T, HW, 0)
    assert torch.equal(out.view(T, 3, HW), x)                            # identity weights: the fp32 value is the input
    _guards_intact("time_conv_out identity", buf, out)
    b8, o8 = _guarded(T * HW * 3, torch.uint8, dev)
    _call(lib, "latte_debug_vae_time_conv_out", x, w, b, o8, T, HW, 1)
    ref = to_uint8(x.cpu()).permute(0, 2, 1)
    diff = o8.view(T, HW, 3).cpu() != ref
    print(f"time_conv_out levels: {int(diff.sum())} of {diff.numel()} bytes differ from the torch fp32 formula")
    assert not bool(diff.any())
    _guards_intact("time_conv_out levels", b8, o8)


# ================================================================================================ packs and convert_split
PACK_SHAPES = [(128, 64), (256, 128)]


def pack_weights(shape, dev):
    """fp32 weights of the usual size with a tenth of them scaled into and below the f16 subnormal range"""
    g = _gen(sum(shape), dev)
    w = torch.randn(*shape, generator=g, device=dev) / math.sqrt(shape[1] * 3)
    tiny = torch.rand(*shape, generator=g, device=dev) < 0.1
    return torch.where(tiny, w * 2.0 ** -(torch.randint(8, 22, shape, generator=g, device=dev).float()), w)


def split16(v):
    hi = v.half()
    return hi, (v - hi.float()).half()


def pack_w_ref(w):
    return split16(w.reshape(w.shape[0], w.shape[1], 9).permute(0, 2, 1).reshape(w.shape[0], -1))


def pack_t_ref(w, swapped=False):
    return split16(w.reshape(w.shape[0], -1) if swapped else w.permute(0, 2, 1).reshape(w.shape[0], -1))


def _bits(t):
    return t.contiguous().view(torch.int16)


def sigmoid_tau(mix):
    return (5 + 2 * abs(mix)) * U32


def test_pack_layouts_restated():
    for Cout, Cin in PACK_SHAPES:
        w = pack_weights((Cout, Cin, 3), CPU)
        hi, lo = pack_t_ref(w)
        assert bool(((hi.float().abs() < 2.0 ** -14) & (hi != 0)).any())                       # f16 subnormals among the packed values
        assert torch.equal(hi.view(Cout, 3, Cin)[5, 2, 7], w[5, 7, 2].half())
        assert not torch.equal(_bits(hi), _bits(pack_t_ref(w, swapped=True)[0]))           # tap and ci swapped: caught bit for bit
        w9 = pack_weights((Cout, Cin, 3, 3), CPU)
        hi9, _ = pack_w_ref(w9)
        assert torch.equal(hi9.view(Cout, 3, 3, Cin)[3, 1, 2, 9], w9[3, 9, 1, 2].half())
        for mix in (-3.0, 0.0, 0.5, 4.0):
            sc = 1.0 / (1.0 + torch.exp(-torch.tensor(mix)))
            hm, lm = pack_t_ref(w * sc)
            want = w.double().permute(0, 2, 1).reshape(Cout, -1) * torch.sigmoid(torch.tensor(mix, dtype=torch.float64))
            _worst("pack_conv_t mix", hm.double() + lm.double(), want, torch.clamp(2.0 ** -22 * want.abs(), min=SUB16 / 2) + sigmoid_tau(mix) * want.abs())


@gpu
@pytest.mark.parametrize("shape", PACK_SHAPES, ids=str)
def test_pack_conv_w_and_t(lib, shape):
    dev = torch.device("cuda")
    Cout, Cin = shape
    for name, taps, ref in (("latte_debug_vae_pack_conv_w", (3, 3), pack_w_ref), ("latte_debug_vae_pack_conv_t", (3,), pack_t_ref)):
        w = pack_weights((Cout, Cin) + taps, dev)
        n = w.numel()
        hi, lo = ref(w)
        for with_lo in (False, True):
            bh, oh = _guarded(n, torch.float16, dev)
            bl, ol = _guarded(n, torch.float16, dev)
            if "conv_t" in name:
                _call(lib, name, w, None, oh, ol if with_lo else None, Cout, Cin)
            else:
                _call(lib, name, w, oh, ol if with_lo else None, Cout, Cin)
            assert torch.equal(_bits(oh), _bits(hi.reshape(-1))), f"{name}: hi differs"
            if with_lo:
                assert torch.equal(_bits(ol), _bits(lo.reshape(-1))), f"{name}: lo differs"
                _guards_intact(name + " lo", bl, ol)
            else:
                assert bool(torch.isnan(ol).all()), f"{name}: wrote out_lo without being asked"
            _guards_intact(name, bh, oh)


@gpu
@pytest.mark.parametrize("mix", [-3.0, 0.0, 0.5, 4.0])
def test_sigmoid_scaled_packs(lib, mix):
    dev = torch.device("cuda")
    mixd = torch.tensor([mix], device=dev)
    sig = torch.sigmoid(torch.tensor(mix, dtype=torch.float64))
    tau = sigmoid_tau(mix)
    for Cout, Cin in PACK_SHAPES:
        w = pack_weights((Cout, Cin, 3), dev)
        n = w.numel()
        bh, oh = _guarded(n, torch.float16, dev)
        bl, ol = _guarded(n, torch.float16, dev)
        _call(lib, "latte_debug_vae_pack_conv_t", w, mixd, oh, ol, Cout, Cin)
        want = w.double().permute(0, 2, 1).reshape(-1) * sig
        r = _worst("pack_conv_t mix", oh.double() + ol.double(), want, torch.clamp(2.0 ** -22 * want.abs(), min=SUB16 / 2) + tau * want.abs())
        rh = _worst("pack_conv_t mix hi", oh.double(), want, torch.clamp(U16 * want.abs(), min=SUB16 / 2) * (1 + 1e-3) + tau * want.abs())
        print(f"pack_conv_t mix {mix} {Cout}x{Cin}: err / bound hi + lo {r:.3g}, hi {rh:.3g}")
        _guards_intact("pack_conv_t mix", bh, oh)
        _guards_intact("pack_conv_t mix lo", bl, ol)
    n = 1000 * 256 + 77
    x = torch.randn(n, generator=_gen(5, dev), device=dev)
    buf, out = _guarded(n, torch.float32, dev)
    _call(lib, "latte_debug_vae_scale_by_sigmoid", x, out, n, mixd)
    want = x.double() * sig
    print(f"scale_by_sigmoid mix {mix}: err / bound {_worst('scale_by_sigmoid', out, want, tau * want.abs()):.3g}")
    _guards_intact("scale_by_sigmoid", buf, out)


@gpu
def test_convert_split(lib):
    dev = torch.device("cuda")
    n = 390 * 256 + 3
    v = pack_weights((n, 1), dev).reshape(-1) * 40.0
    hi, lo = split16(v)
    bh, oh = _guarded(n, torch.float16, dev)
    bl, ol = _guarded(n, torch.float16, dev)
    _call(lib, "latte_debug_convert_split", v, oh, ol, n)
    assert torch.equal(_bits(oh), _bits(hi)) and torch.equal(_bits(ol), _bits(lo))
    _guards_intact("convert_split", bh, oh)
    _guards_intact("convert_split lo", bl, ol)


# ================================================================================================ the hooks' refusals (no GPU needed)
def test_hooks_refuse_what_their_comment_says(lib):
    buf = torch.zeros(256)
    p, null = ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(None)
    bad = lambda rc, word: rc == LATTE_ERR_INVALID and word in lib.latte_last_error()
    assert bad(lib.latte_debug_vae_conv_in(p, p, p, p, 1, 2, 2, 127, null), b"even")
    assert bad(lib.latte_debug_vae_conv_in(p, p, p, p, 1, 2, 2, 0, null), b"even")
    assert bad(lib.latte_debug_vae_conv_out(p, null, p, p, p, 1, 2, 2, 132, 0, null), b"multiple of 8")
    assert bad(lib.latte_debug_vae_conv_out(p, null, p, p, p, 1, 2, 2, 608, 0, null), b"LDS")
    assert bad(lib.latte_debug_vae_conv_out(p, null, p, p, p, 1, 2, 2, 128, 2, null), b"out_mode")
    assert bad(lib.latte_debug_vae_softmax_rows(p, p, 4, 96, 1.0, null), b"L % 64")
    assert bad(lib.latte_debug_vae_softmax_rows(p, p, 4, 4160, 1.0, null), b"L % 64")
    assert bad(lib.latte_debug_vae_time_conv_out(p, p, p, p, 2, 16, 3, null), b"out_mode")
    assert bad(lib.latte_debug_vae_post_quant(null, p, p, p, 1, 4, 1.0, null), b"post_quant")
    assert bad(lib.latte_debug_vae_pack_conv_t(p, null, null, null, 128, 64, null), b"pack_conv_t")
    assert bad(lib.latte_debug_vae_pack_conv_w(p, p, null, 0, 64, null), b"pack_conv_w")
    assert bad(lib.latte_debug_vae_scale_by_sigmoid(p, p, 16, null, null), b"scale_by_sigmoid")
    assert bad(lib.latte_debug_convert_split(p, p, null, 16, null), b"convert_split")
