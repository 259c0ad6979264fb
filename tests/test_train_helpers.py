"""The trainer's helper kernels that no other test reaches one at a time (csrc/train.hip, csrc/pointwise.hip), each through its hook:
unpatchify_bwd, im2col_patch, gather_i64, add_rows, transpose_f32, widen and scale_f32_dev compared EXACTLY (their work is indexing, or one
exactly rounded operation), silu_rows, gated_add, gelu forward / backward and tfreq against fp64 at bounds read off their expressions.
Outputs are NaN-prefilled (or hold the input, for the in-place kernels) inside buffers whose other elements hold a sentinel that must
come back unchanged.  The layout kernels get arange inputs on shapes where no two of BF, G, p, C coincide, so that every misplaced element
and every swapped pair of indices shows.  Sizes: 1, 255, 257 (one thread, a partial block, a second block) and one past each launcher's
block cap (4096 blocks of 256 threads; the GELU launcher's 16384), which only the grid-stride loop reaches.

e = 2^-24.  Bounds:
  silu_rows  |SiLU(x)| (2 |x| + 4) e, the chain of test_bookend_kernels' module docstring; |x| <= 80 (beyond 88 the fast exponential
             overflows and the kernel returns -0 for 1e-37: activations are nowhere near)
  gated_add  x + gate * y: one product and one sum (or one fma), 2 e (|x| + |gate y|)
  gelu fwd   the output is a half: it must be one of the two halves that enclose gelu_tanh in fp64 (faithful rounding) for EVERY half input
             in [-8, 8] -- both zeros, the subnormals and the inputs whose result underflows the type included -- and the nearer one for at
             least 99 % of them.  The fp32 value under the rounding is good to a few e, a half's rounding interval is 2^13 (f16) or 2^16
             (bf16) e wide, so a wrong choice needs the fp64 value within about 2^-10 of a rounding boundary: 0.1 % of inputs.  99 % is
             a condition, not a measurement; test_gelu_restatement_on_the_cpu holds an fp32 numpy restatement to it without a GPU.
  gelu bwd   out = half(d (s + t)), s = sigmoid(2 v), t = x s (1 - s) k, k = 2 v' (kernel comment).  Under the half's rounding -- allowed a
             whole ulp of the type at the reference -- the fp32 value is within
                 e |d| (E_s s (1 + |x| k |1 - 2 s|) + 10 |t| + 2 |s + t|)
             E_s = 2.08 |a| (1 - s) + 5 the relative error of s: a = x (c0 + c1 x^2) is the exponent's argument (x x, the fma, the
             product: 3 e |a| absolute, ln 2 of it relative on exp2, which with the hardware exp2's own ulp (2 e) reaches s through
             e / (1 + e) = 1 - s), then 1 + e (1) and the hardware reciprocal (one ulp: 2); ds reaches the output through d(s + t) / ds =
             1 + x k (1 - 2 s).  t: x s (1), 1 - s (1), their product (1), v' (constants and four operations: 6), the last product (1):
             10.  s + t and the product with d: 2.  This departs from the one-constant form c e |d| (|s| + |t|) in two respects, both
             forced by the expression: the exponent's argument error grows with |x|, and an error of s is amplified by |x| k in t.
             Neither matters beside the half ulp except where gelu' crosses zero (x ~ -0.75), which is what the second term is for.
  tfreq      the CPU-fp32 yardstick of test_bookend_kernels.test_small_linear's timestep mode: four times the deviation of torch's CPU fp32
             evaluation of latte.py:97-117 from its fp64 evaluation.  There it is summed over a row through |W|; here every element
             stands alone and the deviation of a single element can vanish by coincidence, so each element gets the largest deviation
             of its row's half (cos or sin columns of the same t).  t = 0 leaves no slack at all: cos 0 = 1 and sin 0 = 0 exactly.

Worst err / bound per kernel is printed; the figures of the MI355X run are in DESIGN.md section 4.7."""
import math

import numpy as np
import pytest
import torch

from test_bookend_kernels import _call, _rc, _silu64, _sync, _timestep_embedding
from test_train_kernels import DT, TD

gpu = pytest.mark.gpu
U32 = 2.0 ** -24
NAN = float("nan")
SENT = -7.25
PAD = 8
LATTE_ERR_INVALID = 1
CAP = 4096 * 256          # elements one sweep of a 4096-block launch covers
SIZES = [1, 255, 257, CAP + 3]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda")


def _sent(dtype):
    return -7 if dtype == torch.int64 else SENT


def _guarded(n, dev, dtype=torch.float32, fill=None, offset=0):
    """-> (buf, view): n elements PAD + offset into a sentinel-filled buffer; the view holds `fill` (a tensor or a number; default NaN,
    -1 for integers)."""
    buf = torch.full((PAD + offset + n + PAD,), _sent(dtype), device=dev, dtype=dtype)
    view = buf[PAD + offset:PAD + offset + n]
    if torch.is_tensor(fill):
        view.copy_(fill.reshape(-1))
    else:
        view.fill_(fill if fill is not None else (-1 if dtype == torch.int64 else NAN))
    return buf, view


def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _guards_intact(tag, buf, view):
    view.fill_(_sent(buf.dtype))
    assert bool((buf == _sent(buf.dtype)).all()), f"{tag}: wrote outside its range"


def _exact(tag, buf, view, want):
    got = view.clone()
    bad = _bits(got) != _bits(want.reshape(-1).to(got.dtype))
    if bool(bad.any()):
        i = int(torch.nonzero(bad)[0])
        raise AssertionError(f"{tag}: {int(bad.sum())} of {bad.numel()} elements differ; first {i}: got {got[i].item()!r} want "
                             f"{want.reshape(-1)[i].item()!r}")
    _guards_intact(tag, buf, view)
    return got


def _within(tag, got, want, bound):
    want, bound = want.reshape(-1), bound.reshape(-1)
    err = (got.reshape(-1).double() - want).abs()
    bad = ~(err <= bound)
    if bool(bad.any()):
        i = int(torch.nonzero(bad)[0])
        raise AssertionError(f"{tag}: {int(bad.sum())} of {err.numel()} elements out of bound; first {i}: got {float(got.reshape(-1)[i]):.9e} want "
                             f"{float(want[i]):.9e} err {float(err[i]):.3e} > {float(bound[i]):.3e}")
    return float((err / bound.clamp_min(1e-300)).max())


# ------------------------------------------------------------------------------------------------ layout kernels
PATCH_SHAPES = [(3, 5, 2, 8), (2, 3, 4, 3), (1, 7, 1, 5), (33, 32, 2, 8)]      # the last: 1081344 elements, past 4096 blocks


@gpu
@pytest.mark.parametrize("BF,G,p,C", PATCH_SHAPES)
def test_unpatchify_bwd(lib, dev, BF, G, p, C):
    """The inverse of latte.py:297-310 (x.reshape(N, h, w, p, p, c), einsum nhwpqc->nchpwq, reshape(N, c, h p, w p))."""
    H, n = G * p, BF * C * G * p * G * p
    dout = torch.arange(n, device=dev, dtype=torch.float32).view(BF, C, H, H)
    want = dout.view(BF, C, G, p, G, p).permute(0, 2, 4, 3, 5, 1).reshape(BF * G * G, p * p * C)       # n c h p w q -> n h w p q c
    buf, view = _guarded(n, dev)
    _call(lib, "latte_debug_unpatchify_bwd", dout, view, BF, G, p, C)
    _exact(f"unpatchify_bwd {(BF, G, p, C)}", buf, view, want)


@gpu
@pytest.mark.parametrize("BF,G,p,C", PATCH_SHAPES)
def test_im2col_patch(lib, dev, BF, G, p, C):
    """Row m = (bf, gh, gw) holds its patch in Conv2d's weight order (c, i, j): what x_embedder.proj contracts with."""
    H, n = G * p, BF * C * G * p * G * p
    x = torch.arange(n, device=dev, dtype=torch.float32).view(BF, C, H, H)
    want = x.view(BF, C, G, p, G, p).permute(0, 2, 4, 1, 3, 5).reshape(BF * G * G, C * p * p)
    if p > 1:       # the restatement is Conv2d's: unfold is torch's own im2col of a k = s = p convolution
        assert torch.equal(want, torch.nn.functional.unfold(x, p, stride=p).transpose(1, 2).reshape(BF * G * G, C * p * p))
    buf, view = _guarded(n, dev)
    _call(lib, "latte_debug_im2col_patch", x, view, BF, G, p, C)
    _exact(f"im2col_patch {(BF, G, p, C)}", buf, view, want)


@gpu
def test_patch_layout_hooks_refuse(lib, dev):
    z = torch.zeros(64, device=dev)
    for name in ("latte_debug_unpatchify_bwd", "latte_debug_im2col_patch"):
        assert _rc(lib, name, z, z.clone(), 1, 2, 2, 4) == 0
        _sync(dev)
        for args in ((0, 2, 2, 4), (1, 0, 2, 4), (1, 2, 0, 4), (1, 2, 2, 0), (1, 2, 65536, 1)):
            assert _rc(lib, name, z, z.clone(), *args) == LATTE_ERR_INVALID, (name, args)
        assert _rc(lib, name, None, z, 1, 2, 2, 4) == LATTE_ERR_INVALID and _rc(lib, name, z, None, 1, 2, 2, 4) == LATTE_ERR_INVALID


# ------------------------------------------------------------------------------------------------ exact one-liners
@gpu
@pytest.mark.parametrize("n", SIZES)
def test_gather_i64(lib, dev, n):
    g = torch.Generator(dev).manual_seed(n)
    table = torch.randint(-2 ** 62, 2 ** 62, (1000,), generator=g, device=dev, dtype=torch.int64)     # values that need all 64 bits
    idx = torch.randint(0, 1000, (n,), generator=g, device=dev, dtype=torch.int64)
    buf, view = _guarded(n, dev, torch.int64)
    _call(lib, "latte_debug_gather_i64", table, idx, view, n)
    _exact(f"gather_i64 n{n}", buf, view, table[idx])
    assert _rc(lib, "latte_debug_gather_i64", table, idx, view, 0) == LATTE_ERR_INVALID


@gpu
@pytest.mark.parametrize("n", SIZES)
def test_add_rows(lib, dev, n):
    g = torch.Generator(dev).manual_seed(n)
    a, b = torch.randn(n, generator=g, device=dev), torch.randn(n, generator=g, device=dev) * 3
    buf, view = _guarded(n, dev, fill=a)
    sbuf, src = _guarded(n, dev, fill=b)
    _call(lib, "latte_debug_add_rows", view, src, n)
    _exact(f"add_rows n{n}", buf, view, a + b)                 # one fp32 addition per element: the same bits
    _exact(f"add_rows n{n}: src", sbuf, src, b)
    assert _rc(lib, "latte_debug_add_rows", view, src, 0) == LATTE_ERR_INVALID


@gpu
@pytest.mark.parametrize("rows,cols", [(1, 1), (15, 17), (257, 1), (1, 257), (33, 95), (1031, 1021)])      # the last: 1052651 > 4096 x 256
def test_transpose_f32(lib, dev, rows, cols):
    x = torch.arange(rows * cols, device=dev, dtype=torch.float32).view(rows, cols)
    buf, view = _guarded(rows * cols, dev)
    _call(lib, "latte_debug_transpose_f32", x, view, rows, cols)
    _exact(f"transpose_f32 {rows}x{cols}", buf, view, x.t().contiguous())
    for args in ((x, view, 0, cols), (x, view, rows, 0), (x, x, rows, cols), (None, view, rows, cols)):
        assert _rc(lib, "latte_debug_transpose_f32", *args) == LATTE_ERR_INVALID


@gpu
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_widen(lib, dev, dt):
    """Every bit pattern of the type except the NaNs (zeros, subnormals, infinities included), tiled past the block cap."""
    allbits = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).to(dev)
    allbits = allbits[~torch.isnan(allbits.view(TD[dt]))]
    for n in SIZES + [allbits.numel()]:
        src = allbits.repeat(n // allbits.numel() + 1)[-n:].contiguous()
        buf, view = _guarded(n, dev)
        _call(lib, "latte_debug_widen", src, view, n, DT[dt])
        _exact(f"widen {dt} n{n}", buf, view, src.view(TD[dt]).float())
    assert _rc(lib, "latte_debug_widen", src, view, 0, DT[dt]) == LATTE_ERR_INVALID
    assert _rc(lib, "latte_debug_widen", src, view, 4, 7) == LATTE_ERR_INVALID


@gpu
@pytest.mark.parametrize("n", SIZES)
def test_scale_f32_dev(lib, dev, n):
    """x 2^14 and x 1 / 2^14 are exact on normal values whose result is normal; the round trip is the identity."""
    g = torch.Generator(dev).manual_seed(n)
    x = (10.0 ** (torch.rand(n, generator=g, device=dev, dtype=torch.float64) * 60 - 30)).float() * torch.where(torch.rand(n, generator=g, device=dev) < 0.5, -1.0, 1.0)
    sbuf, s = _guarded(1, dev, fill=2.0 ** 14)
    for first in (0, 1):
        buf, view = _guarded(n, dev, fill=x)
        _call(lib, "latte_debug_scale_f32_dev", view, s, first, n)
        assert torch.equal(_bits(view), _bits(x * 2.0 ** 14 if first == 0 else x / 2.0 ** 14)), f"scale_f32_dev n{n} inverse {first}"
        _call(lib, "latte_debug_scale_f32_dev", view, s, 1 - first, n)
        _exact(f"scale_f32_dev n{n}: round trip from inverse {first}", buf, view, x)
    assert float(s[0]) == 2.0 ** 14
    _guards_intact("scale_f32_dev: scale", sbuf, s)
    for args in ((view, s, 0, 0), (view, s, 2, n), (None, s, 0, n), (view, None, 0, n)):
        assert _rc(lib, "latte_debug_scale_f32_dev", *args) == LATTE_ERR_INVALID


# ------------------------------------------------------------------------------------------------ silu_rows
@gpu
@pytest.mark.parametrize("n", SIZES)
def test_silu_rows(lib, dev, n):
    g = torch.Generator(dev).manual_seed(n)
    x = torch.randn(n, generator=g, device=dev) * 3
    edge = torch.tensor([0.0, -0.0, 80.0, -80.0, 20.0, -20.0, 1e-30, -1e-30, 1.0, -1.2785], device=dev)
    k = min(n, edge.numel())
    x[:k] = edge[:k]
    want, bound = _silu64(x)
    obuf, out = _guarded(n, dev)
    _call(lib, "latte_debug_silu_rows", x, out, n)
    ratio = _within(f"silu_rows n{n}", out, want, bound)
    ibuf, inp = _guarded(n, dev, fill=x)
    _call(lib, "latte_debug_silu_rows", inp, inp, n)                     # in place, as engine.cpp calls it
    assert torch.equal(_bits(inp), _bits(out)), f"silu_rows n{n}: in place differs from out of place"
    _guards_intact("silu_rows out", obuf, out)
    _guards_intact("silu_rows in place", ibuf, inp)
    assert _rc(lib, "latte_debug_silu_rows", x, out, 0) == LATTE_ERR_INVALID
    print(f"silu_rows n{n}: worst err / bound {ratio:.3f}")


# ------------------------------------------------------------------------------------------------ gated_add
@gpu
@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("D,rps", [(128, 32), (128, 256), (1152, 32), (1152, 256), (1024, 1376)])     # the last: 4128 x 1024 > 4096 x 256 x 4
def test_gated_add(lib, dev, D, rps, dt):
    """Three samples of rps rows with different gates (rows of a [3, 6 D] modulation buffer, as the trainer passes them: the gate chunk
    starts 2 D floats into each row)."""
    M = 3 * rps
    g = torch.Generator(dev).manual_seed(D + rps)
    x = torch.randn(M, D, generator=g, device=dev)
    y = (torch.randn(M, D, generator=g, device=dev) * 2).to(TD[dt])
    mod = torch.randn(3, 6 * D, generator=g, device=dev)
    gate = mod[:, 2 * D:3 * D]
    gy = gate.double().repeat_interleave(rps, 0) * y.double()
    want = x.double() + gy
    bound = 2 * U32 * (x.double().abs() + gy.abs())
    buf, view = _guarded(M * D, dev)
    _call(lib, "latte_debug_gated_add", x, y, gate, 6 * D, view, M, D, rps, DT[dt])
    ratio = _within(f"gated_add D{D} rps{rps} {dt}", view, want, bound)
    _guards_intact("gated_add", buf, view)
    print(f"gated_add D{D} rps{rps} {dt}: worst err / bound {ratio:.3f}")


@gpu
def test_gated_add_refuses(lib, dev):
    x, y, gt = torch.zeros(64 * 128 + 4, device=dev), torch.zeros(64 * 128 + 4, device=dev, dtype=torch.float16), torch.ones(2 * 128 + 4, device=dev)
    ok = lambda **k: _rc(lib, "latte_debug_gated_add", k.get("x", x), k.get("y", y), k.get("g", gt), k.get("gs", 128), k.get("o", x.clone()),
                         k.get("M", 64), k.get("D", 128), k.get("rps", 32), k.get("dt", 1))
    assert ok() == 0
    _sync(dev)
    for k in (dict(D=126), dict(rps=0), dict(gs=64), dict(gs=130), dict(M=0), dict(dt=5), dict(x=x[1:]), dict(g=gt[1:]), dict(o=x[1:]),
              dict(y=y[1:]), dict(x=None), dict(y=None)):
        assert ok(**k) == LATTE_ERR_INVALID, k


# ------------------------------------------------------------------------------------------------ GELU
C0, C1 = -2.3022082, -0.10294324           # device_util.h: gelu_sig's exponent is exp2(x (C0 + C1 x^2))


def _gelu64(x):
    """-> gelu_tanh, its sigmoid factor s, and k = 2 v' of the kernel comment, in fp64."""
    x = x.double()
    v = math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)
    s = torch.sigmoid(2.0 * v)
    k = 2.0 * math.sqrt(2.0 / math.pi) * (1.0 + 3 * 0.044715 * x * x)
    return x * s, s, k


def _half_inputs(dt, dev):
    """every value of the type in [-8, 8] -- both zeros and the subnormals among them -- padded with zeros to a multiple of 4."""
    allbits = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16)
    v = allbits.view(TD[dt])
    keep = allbits[v.double().abs() <= 8.0]            # (NaN compares false)
    keep = torch.cat([keep, torch.zeros((-keep.numel()) % 4, dtype=torch.int16)])
    return keep.to(dev).view(TD[dt])


def _half_table(dt, dev):
    """the type's finite values in ascending order, fp64."""
    allbits = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16)
    v = allbits.view(TD[dt]).double()
    return torch.unique(v[torch.isfinite(v)]).to(dev)


def _faithful(tag, got, ref, table):
    """got (half) must be one of the two table values enclosing ref; -> share of elements that took the nearer one."""
    hi_i = torch.searchsorted(table, ref.contiguous())
    hi = table[hi_i]
    lo = torch.where(hi == ref, hi, table[(hi_i - 1).clamp_min(0)])
    gd = got.double()
    bad = ~((gd == lo) | (gd == hi))
    if bool(bad.any()):
        i = int(torch.nonzero(bad)[0])
        raise AssertionError(f"{tag}: {int(bad.sum())} of {bad.numel()} outputs are not a neighbour of the fp64 value; first {i}: got "
                             f"{float(gd[i])!r}, fp64 {float(ref[i])!r} lies in [{float(lo[i])!r}, {float(hi[i])!r}]")
    return float(((gd - ref).abs() <= torch.minimum((lo - ref).abs(), (hi - ref).abs())).double().mean())


def _gelu_f32(x):
    """gelu_kernel<DT, false> in numpy fp32: x * rcp(1 + exp2(x * fma(x x, C1, C0)))."""
    f = np.float32
    x = x.astype(f)
    p = ((x * x).astype(np.float64) * float(f(C1)) + float(f(C0))).astype(f)
    with np.errstate(over="ignore"):          # exp2 -> inf -> reciprocal 0 is the kernel's path for x << 0
        return x * (f(1.0) / (f(1.0) + np.exp2(p * x)))


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_gelu_restatement_on_the_cpu(dt):
    """No GPU: the restatement meets the forward test's two conditions on the forward test's inputs."""
    cpu = torch.device("cpu")
    x = _half_inputs(dt, cpu)
    out = torch.from_numpy(_gelu_f32(x.float().numpy())).to(TD[dt])
    share = _faithful(f"gelu restatement {dt}", out, _gelu64(x)[0], _half_table(dt, cpu))
    print(f"gelu restatement {dt}: {x.numel()} inputs, nearest for {share:.5f}")
    assert share >= 0.99


@gpu
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_gelu_forward(lib, dev, dt):
    x = _half_inputs(dt, dev)
    n = x.numel()
    assert n % 4 == 0
    buf, view = _guarded(n, dev, TD[dt])
    _call(lib, "latte_debug_gelu", x, None, view, n, 0, DT[dt])
    got = view.clone()
    _guards_intact(f"gelu forward {dt}", buf, view)
    assert bool(torch.isfinite(got).all())
    share = _faithful(f"gelu forward {dt}", got, _gelu64(x)[0], _half_table(dt, dev))
    print(f"gelu forward {dt}: {n} inputs, nearest for {share:.5f}")
    assert share >= 0.99
    neg0 = _bits(x) == -32768
    assert bool((_bits(got)[neg0] == -32768).all()), "gelu(-0) must be -0"


@gpu
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_gelu_past_the_block_cap(lib, dev, dt):
    """16384 blocks x 256 threads x 4 elements = 16777216: forward and backward on 16777216 + 4 x 259 elements equal, bit for bit, the same
    kernels on the first and the last 2^20 elements alone (every element depends on its own input only)."""
    n, k = 16384 * 256 * 4 + 4 * 259, 2 ** 20
    g = torch.Generator(dev).manual_seed(5)
    x = (torch.randn(n, generator=g, device=dev) * 2).to(TD[dt])
    d = torch.randn(n, generator=g, device=dev).to(TD[dt])
    for bwd in (0, 1):
        buf, view = _guarded(n, dev, TD[dt])
        _call(lib, "latte_debug_gelu", x, d if bwd else None, view, n, bwd, DT[dt])
        for sl in (slice(0, k), slice(n - k, n)):
            part = torch.full((k,), NAN, device=dev, dtype=TD[dt])
            _call(lib, "latte_debug_gelu", x[sl].clone(), d[sl].clone() if bwd else None, part, k, bwd, DT[dt])
            assert torch.equal(_bits(view[sl]), _bits(part)), f"gelu bwd {bwd} {dt}: elements {sl} differ from the short launch"
        assert bool(torch.isfinite(view.float()).all())
        _guards_intact(f"gelu bwd {bwd} {dt} large", buf, view)


def _ulp_half(ref, dt):
    """one ulp of the type at |ref| (f16: not below its subnormal spacing 2^-24)."""
    e = torch.floor(torch.log2(ref.abs().clamp_min(1e-300)))
    return torch.exp2(e - 10).clamp_min(2.0 ** -24) if dt == "f16" else torch.exp2(e - 7)


@gpu
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_gelu_backward(lib, dev, dt):
    x = _half_inputs(dt, dev)
    n = x.numel()
    g = torch.Generator(dev).manual_seed(11)
    d = (torch.randn(n, generator=g, device=dev, dtype=torch.float64) * 10.0 ** (torch.rand(n, generator=g, device=dev, dtype=torch.float64) * 4 - 3)).to(TD[dt])
    xd, dd = x.double(), d.double()
    _, s, k = _gelu64(x)
    t = xd * s * (1 - s) * k
    want = dd * (s + t)
    a = (xd * (C0 + C1 * xd * xd)).abs()
    e_s = 2.08 * a * (1 - s) + 5
    bound = _ulp_half(want, dt) + U32 * dd.abs() * (e_s * s * (1 + xd.abs() * k * (1 - 2 * s).abs()) + 10 * t.abs() + 2 * (s + t).abs())
    buf, view = _guarded(n, dev, TD[dt])
    _call(lib, "latte_debug_gelu", x, d, view, n, 1, DT[dt])
    ratio = _within(f"gelu backward {dt}", view, want, bound)
    near = (xd + 0.75).abs() < 0.05                      # where gelu' crosses zero: the half ulp vanishes with the reference
    ratio0 = float((((view.double() - want).abs() / bound)[near]).max())
    ibuf, inp = _guarded(n, dev, TD[dt], fill=d)
    _call(lib, "latte_debug_gelu", x, inp, inp, n, 1, DT[dt])             # in place, as the trainer runs it
    assert torch.equal(_bits(inp), _bits(view)), f"gelu backward {dt}: in place differs from out of place"
    _guards_intact(f"gelu backward {dt}", buf, view)
    _guards_intact(f"gelu backward {dt} in place", ibuf, inp)
    print(f"gelu backward {dt}: worst err / bound {ratio:.3f}, near the zero of gelu' {ratio0:.3f}")


@gpu
def test_gelu_refuses(lib, dev):
    h = torch.zeros(16, device=dev, dtype=torch.float16)
    o = torch.zeros(16, device=dev, dtype=torch.float16)
    assert _rc(lib, "latte_debug_gelu", h, None, o, 8, 0, 1) == 0 and _rc(lib, "latte_debug_gelu", h, h, o, 8, 1, 1) == 0
    _sync(dev)
    for args in ((h, None, o, 6, 0, 1), (h, None, o, 0, 0, 1), (h, None, o, 8, 1, 1), (h, None, o, 8, 2, 1), (h, None, o, 8, 0, 9),
                 (None, None, o, 8, 0, 1), (h, None, None, 8, 0, 1), (h[1:], None, o, 8, 0, 1)):
        assert _rc(lib, "latte_debug_gelu", *args) == LATTE_ERR_INVALID, args[3:]


# ------------------------------------------------------------------------------------------------ tfreq
@gpu
def test_tfreq(lib, dev):
    t = torch.tensor([0, 1, 500, 999], dtype=torch.int64)
    e64 = _timestep_embedding(t, 256, torch.float64)
    dev32 = (_timestep_embedding(t, 256, torch.float32).double() - e64).abs().view(4, 2, 128)
    bound = (4 * dev32.amax(dim=2, keepdim=True)).expand(4, 2, 128).reshape(4, 256).to(dev)
    buf, view = _guarded(4 * 256, dev)
    _call(lib, "latte_debug_tfreq", t.to(dev), view, 4)
    got = view.view(4, 256).clone()
    assert got[0].tolist() == [1.0] * 128 + [0.0] * 128, "t = 0: [cos | sin] = [1 | 0] exactly"
    ratio = _within("tfreq", got[1:], e64[1:].to(dev), bound[1:])
    _within("tfreq t 0", got[:1], e64[:1].to(dev), bound[:1])
    _guards_intact("tfreq", buf, view)
    assert _rc(lib, "latte_debug_tfreq", t.to(dev), view, 0) == LATTE_ERR_INVALID
    print(f"tfreq: worst err / bound {ratio:.3f} (rows t = 1, 500, 999: " + ", ".join(
        f"{float(((got[i].double() - e64[i].to(dev)).abs() / bound[i]).max()):.3f}" for i in (1, 2, 3)) + ")")
