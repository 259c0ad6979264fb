"""The denoiser's fp32 bookend kernels (csrc/pointwise.hip) one at a time through their hooks: small_linear (plain, SiLU and timestep
input), patch_embed, final_layer (P == 32 and generic path), text_proj, gated_split_reduce, adaln_single, cond_rows and mask_bias, each
against an fp64 evaluation of the same expression on the same fp32 inputs, per element, the output NaN-prefilled inside a buffer whose
every other element holds a sentinel that must come back bit for bit.

Bounds are first order, e = 2^-24: a chain of n fp32 operations over terms a_i b_i is allowed n e sum |a_i| |b_i|, n read off the kernel and
written beside each case.  SiLU(x) = x / (1 + __expf(-x)), __expf(y) = exp2(y log2(e)) on the hardware exponential: the rounded constant
and the rounded product move the exponent by 2 e |y| log2(e), a factor 2 e |x| on the result; the hardware exp2 is good to one ulp = 2 e;
the add and the divide round once each: |SiLU(x)| (2 |x| + 4) e.  The timestep sinusoid is the one place where a library function's
error is multiplied by a large argument; its yardstick is described in test_small_linear."""
import math

import pytest
import torch

from latte_amd._lib import check, ptr, stream_ptr

pytestmark = pytest.mark.gpu
U32 = 2.0 ** -24
NAN = float("nan")
SENT = -7.25
PAD = 8


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda")


def _sync(dev):
    if dev.type == "cuda":
        torch.cuda.synchronize()


def _call(lib, name, *args):
    """One hook call: tensors go as device pointers, None as NULL, the current stream last."""
    check(getattr(lib, name)(*[ptr(a) if (a is None or torch.is_tensor(a)) else a for a in args], stream_ptr()))
    for a in args:
        if torch.is_tensor(a):
            _sync(a.device)
            return


def _rc(lib, name, *args):
    return getattr(lib, name)(*[ptr(a) if (a is None or torch.is_tensor(a)) else a for a in args], stream_ptr())


def _out(rows, cols, stride, dev):
    """-> (buf, view): a NaN [rows, cols] view, rows `stride` floats apart, PAD floats into a buffer that is SENT everywhere else."""
    buf = torch.full((PAD + rows * stride + PAD,), SENT, device=dev)
    view = buf[PAD:PAD + rows * stride].view(rows, stride)[:, :cols]
    view.fill_(NAN)
    return buf, view


def _finish(tag, buf, view, want, bound):
    """every owned element written and within its bound, everything else untouched."""
    got = view.clone()
    assert bool(torch.isfinite(got).all()), f"{tag}: {int((~torch.isfinite(got)).sum())} owned elements not written"
    view.fill_(SENT)
    assert bool((buf.view(torch.int32) == torch.tensor([SENT], device=buf.device).view(torch.int32)).all()), f"{tag}: wrote outside its range"
    err = (got.double() - want).abs()
    bad = ~(err <= bound)
    ratio = float((err / bound.clamp_min(1e-300)).max())
    if bool(bad.any()):
        i = tuple(int(x) for x in torch.nonzero(bad)[0])
        raise AssertionError(f"{tag}: {int(bad.sum())} of {err.numel()} elements out of bound; first {i}: got {float(got[i]):.7e} want "
                             f"{float(want[i]):.7e} err {float(err[i]):.3e} > {float(bound[i]):.3e}; worst err / bound {ratio:.3f}")
    return got, ratio


def _silu64(x):
    """-> SiLU in fp64 and the bound of the kernels' fp32 SiLU (module docstring)."""
    x = x.double()
    s = x / (1.0 + torch.exp(-x))
    return s, s.abs() * (2 * x.abs() + 4) * U32


def _rand(shape, g, dev, scale=1.0):
    return torch.randn(shape, generator=g, device=dev) * scale


# ------------------------------------------------------------------------------------------------ small_linear
def _timestep_embedding(t, K, dtype):
    """latte.py:97-117 in `dtype`: freqs = exp(-ln(1e4) arange(half) / half), emb = [cos(t freqs) | sin(t freqs)]."""
    half = K // 2
    freqs = torch.exp(-math.log(10000) * torch.arange(half, dtype=torch.float32).to(dtype) / half)
    args = t[:, None].to(dtype) * freqs[None]
    return torch.cat([torch.cos(args), torch.sin(args)], dim=-1)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("N", [5, 128, 768])      # 5: the last block keeps one wave of four
@pytest.mark.parametrize("K", [128, 256, 1152])
def test_small_linear(lib, dev, K, N, B):
    """out[b, n] = bias[n] + sum_k f(in[b, k]) W[n, k] (+ table[idx[b], n]), out rows out_stride = N + 3 apart.  Chain: a lane adds K / 64
    products (fma), the wave butterfly 6 more, then the bias and the table row: n = K / 64 + 8, on sum |f| |W| + |bias| + |table|; SiLU mode
    adds sum_k dSiLU(in_k) |W_nk| (module docstring).  Timestep mode: t in {0, 1, 500, 999} at B = 3 (+ 999 again), t = 999 at B = 1;
    the yardstick for the device expf / cosf / sinf, whose errors meet arguments up to 999: the ROCm documentation on the build
    machine states no ulp figures for them, so the deviation of torch's CPU fp32 evaluation of the reference formula (latte.py:97-117)
    from its fp64 evaluation is taken per embedding element for the same t, and four times it -- two independent fp32 libms may err in
    opposite directions -- goes through |W| into the bound: 4 sum_k |emb32_k - emb64_k| |W_nk| + n e (sum |emb| |W| + |bias|).
    Worst err / bound observed on the MI355X: recorded in DESIGN.md section 4.6."""
    g = torch.Generator(dev).manual_seed(K * 7 + N * 3 + B)
    W, bias = _rand((N, K), g, dev, K ** -0.5), _rand((N,), g, dev)
    x = _rand((B, K), g, dev, 2.0)
    table, idx = _rand((4, N), g, dev), torch.tensor([2, 2, 0][:B], device=dev)            # a repeated row among them
    chain = K // 64 + 8
    Wd = W.double()
    worst = {}
    for mode, use_table in ((0, False), (0, True), (1, False), (2, False)):
        t = None
        if mode == 2:
            t = torch.tensor([999] if B == 1 else [0, 1, 500], device=dev, dtype=torch.int64)
            f = _timestep_embedding(t.cpu(), K, torch.float64).to(dev)
            df = 4 * (_timestep_embedding(t.cpu(), K, torch.float32).double().to(dev) - f).abs()
        elif mode == 1:
            f, df = _silu64(x)
        else:
            f, df = x.double(), torch.zeros_like(x, dtype=torch.float64)
        want = f @ Wd.T + bias.double()
        mag = f.abs() @ Wd.abs().T + bias.double().abs()
        if use_table:
            want, mag = want + table.double()[idx], mag + table.double()[idx].abs()
        bound = df @ Wd.abs().T + chain * U32 * mag
        buf, view = _out(B, N, N + 3, dev)
        _call(lib, "latte_debug_small_linear", mode, None if mode == 2 else x, t, W, bias, table if use_table else None,
              idx if use_table else None, view, B, N, K, N + 3)
        _, worst[mode, use_table] = _finish(f"small_linear mode {mode} table {use_table} K{K} N{N} B{B}", buf, view, want, bound)
    if B == 3:                                    # t = 999 beside 0: the remaining timestep of the list
        t = torch.tensor([999, 0, 999], device=dev, dtype=torch.int64)
        f = _timestep_embedding(t.cpu(), K, torch.float64).to(dev)
        df = 4 * (_timestep_embedding(t.cpu(), K, torch.float32).double().to(dev) - f).abs()
        buf, view = _out(B, N, N + 3, dev)
        _call(lib, "latte_debug_small_linear", 2, None, t, W, bias, None, None, view, B, N, K, N + 3)
        _, r = _finish(f"small_linear timestep 999 K{K} N{N}", buf, view, f @ Wd.T + bias.double(),
                       df @ Wd.abs().T + chain * U32 * (f.abs() @ Wd.abs().T + bias.double().abs()))
        worst[2, False] = max(worst[2, False], r)
    print(f"small_linear K{K} N{N} B{B}: worst err / bound " + ", ".join(f"mode {m}{'+table' if tb else ''} {r:.3f}" for (m, tb), r in worst.items()))


def test_small_linear_refuses(lib, dev):
    z = torch.zeros(4 * 256, device=dev)
    t = torch.zeros(1, device=dev, dtype=torch.int64)
    ok = lambda **kw: _rc(lib, "latte_debug_small_linear", kw.get("mode", 0), kw.get("x", z), kw.get("t", None), z, z, kw.get("tab", None), None, z, 1, 4,
                          kw.get("K", 128), kw.get("stride", 4))
    assert ok() == 0
    _sync(dev)
    for kw in (dict(K=64), dict(K=1280), dict(stride=3), dict(mode=2), dict(mode=3), dict(x=None), dict(tab=z)):
        assert ok(**kw) == 1, kw
    assert ok(mode=2, t=t, x=None, K=256) == 0
    _sync(dev)


# ------------------------------------------------------------------------------------------------ patch_embed
@pytest.mark.parametrize("C,H,p,D,BF", [(4, 8, 2, 128, 3), (4, 16, 2, 384, 2), (4, 16, 8, 128, 5), (3, 12, 4, 256, 3)])
def test_patch_embed(lib, dev, C, H, p, D, BF):
    """out[tok, :] = Wt^T pixels(tok) + bias + pos[tok % T, :] (Conv2d with kernel = stride = p, then the position table).  The kernel works
    on blocks of 16 tokens: (4, 16, 8, 128) runs 5 frames of T = 4 tokens and (3, 12, 4, 256) 3 frames of T = 9, so their last block keeps 4
    and 11 tokens; at T = 16 and T = 64 every whole number of frames is a multiple of 16, those two shapes check the addressing and the
    second 128-feature block column (D = 384) on full blocks, over several frames so that tok % T wraps.  Chain: K = C p p fma and two
    adds, n = K + 2."""
    G = H // p
    T, K = G * G, C * p * p
    ntok = BF * T
    assert ntok % 16 or T % 16 == 0
    g = torch.Generator(dev).manual_seed(C * 1000 + H * 10 + p)
    x = _rand((BF, C, H, H), g, dev)
    Wt, bias, pos = _rand((K, D), g, dev, K ** -0.5), _rand((D,), g, dev), _rand((T, D), g, dev)
    pix = x.double().view(BF, C, G, p, G, p).permute(0, 2, 4, 1, 3, 5).reshape(ntok, K)       # k = (c p + i) p + j
    posr = pos.double()[torch.arange(ntok, device=dev) % T]
    want = pix @ Wt.double() + bias.double() + posr
    bound = (K + 2) * U32 * (pix.abs() @ Wt.double().abs() + bias.double().abs() + posr.abs())
    buf, view = _out(ntok, D, D, dev)
    _call(lib, "latte_debug_patch_embed", x, Wt, bias, pos, view, BF, C, H, p, D)
    _, r = _finish(f"patch_embed C{C} H{H} p{p} D{D} BF{BF}", buf, view, want, bound)
    print(f"patch_embed C{C} H{H} p{p} D{D} BF{BF} ({ntok} tokens): worst err / bound {r:.3f}")


def test_patch_embed_refuses(lib, dev):
    z = torch.zeros(4096, device=dev)
    f = lambda BF=1, C=4, H=8, p=2, D=128: _rc(lib, "latte_debug_patch_embed", z, z, z, z, z, BF, C, H, p, D)
    assert f() == 0
    _sync(dev)
    assert f(D=192) == 1 and f(D=64) == 1          # D not a multiple of 128
    assert f(H=9) == 1                             # H % p != 0
    assert f(C=17, H=8, p=8) == 1                  # 16 x 1088 floats of dynamic LDS: above the 64 KiB default
    assert f(BF=0) == 1


# ------------------------------------------------------------------------------------------------ final_layer
@pytest.mark.parametrize("mod_stride_mult", [0, 6])
@pytest.mark.parametrize("rps", [4, 36])
@pytest.mark.parametrize("p,Cout", [(2, 8), (2, 4), (4, 8)])      # P = p p Cout = 32 (its own path), 16 and 128 (generic path)
@pytest.mark.parametrize("D", [128, 384, 1152])
def test_final_layer(lib, dev, D, p, Cout, rps, mod_stride_mult):
    """y = LN(x) (1 + scale[s]) + shift[s], s = row // rows_per_sample; out = unpatchify(y Wt + bias), einsum('nhwpqc->nchpwq').  M = 36
    rows (4 frames of a 3 x 3 token grid): the fifth 8-row block keeps 4 rows, and rows_per_sample 4 puts two samples into every block, 36 one.
    mod_stride 0: one modulation row for every sample.  The output is NaN-prefilled and has exactly M P elements, so "all finite, nothing
    else touched" is "every pixel written once".

    Bound.  LayerNorm chain c1 = D / 64 + 7 (D / 64 values per lane, the 6-level butterfly, the scaling): dmu = c1 e mean|x|;  d = x - mu:
    dd = e |d| + dmu;  var = mean d^2: dvar = (c1 + 3) e var + 2 mean|d| dmu;  rstd: relative rr = dvar / (2 (var + eps)) + 3 e (add, sqrt,
    divide);  y: dy = |d rstd (1 + scale)| (rr + 4 e) + dmu rstd |1 + scale| + e |y|.  Linear: sum_k dy_k |Wt_kj| + n e (sum_k |y_k| |Wt_kj|
    + |bias_j|), n = D / 8 + 5 on the P == 32 path (an eighth of the products per thread, the half-wave shuffle, three adds across the
    waves, the bias), n = D / 4 + 3 on the generic path (four interleaved chains, two adds, the bias)."""
    Gd, F = 3, 4
    T, H, P = Gd * Gd, Gd * p, p * p * Cout
    M = F * T
    assert M % 8 and M % rps == 0
    S = M // rps
    ms = mod_stride_mult * D
    g = torch.Generator(dev).manual_seed(D + 17 * p + Cout + rps)
    x = _rand((M, D), g, dev) * (0.5 + 1.5 * torch.rand(M, 1, generator=g, device=dev)) + _rand((M, 1), g, dev)
    mod = _rand((max(S * ms, 2 * D),), g, dev, 0.5)
    shift, scale = mod, mod[D:]          # the engines' layout: scale D floats behind shift in the same row
    Wt, bias = _rand((D, P), g, dev, D ** -0.5), _rand((P,), g, dev)
    smp = torch.arange(M, device=dev) // rps
    col = torch.arange(D, device=dev)
    sh = mod.double()[(smp * ms)[:, None] + col[None]]
    sc = mod.double()[(smp * ms)[:, None] + D + col[None]]
    xd = x.double()
    mu = xd.mean(1, keepdim=True)
    d = xd - mu
    var = (d * d).mean(1, keepdim=True)
    rstd = (var + 1e-6) ** -0.5
    y = d * rstd * (1 + sc) + sh
    c1 = D // 64 + 7
    dmu = c1 * U32 * xd.abs().mean(1, keepdim=True)
    dvar = (c1 + 3) * U32 * var + 2 * d.abs().mean(1, keepdim=True) * dmu
    rr = dvar / (2 * (var + 1e-6)) + 3 * U32
    dy = (d * rstd * (1 + sc)).abs() * (rr + 4 * U32) + dmu * rstd * (1 + sc).abs() + U32 * y.abs()
    n = D // 8 + 5 if P == 32 else D // 4 + 3
    Wd = Wt.double()
    tok = y @ Wd + bias.double()
    btok = dy @ Wd.abs() + n * U32 * (y.abs() @ Wd.abs() + bias.double().abs())
    unpatch = lambda v: torch.einsum("nhwpqc->nchpwq", v.view(F, Gd, Gd, p, p, Cout)).reshape(F * Cout * H, H)
    buf, view = _out(F * Cout * H, H, H, dev)
    _call(lib, "latte_debug_final_layer", x, shift, scale, ms, Wt, bias, view, M, D, rps, T, p, Cout, H)
    _, r = _finish(f"final_layer D{D} p{p} Cout{Cout} rps{rps} mod_stride {ms}", buf, view, unpatch(tok), unpatch(btok))
    print(f"final_layer D{D} p{p} Cout{Cout} rps{rps} mod_stride {ms}: worst err / bound {r:.3f}")


def test_final_layer_refuses(lib, dev):
    z = torch.zeros(8192, device=dev)
    f = lambda M=9, D=128, rps=9, T=9, p=2, H=6, ms=0: _rc(lib, "latte_debug_final_layer", z, z, z, ms, z, z, z, M, D, rps, T, p, 8, H)
    assert f() == 0
    _sync(dev)
    assert f(D=192) == 1 and f(D=640) == 1     # not a multiple of 128; a multiple the kernel is not instantiated for
    assert f(H=7) == 1                         # H % p != 0
    assert f(rps=0) == 1 and f(rps=-4) == 1
    assert f(T=8) == 1 and f(M=10) == 1 and f(ms=3) == 1


# ------------------------------------------------------------------------------------------------ text_proj
@pytest.mark.parametrize("N", [6, 128])
@pytest.mark.parametrize("B", [1, 8, 9])          # 9: a second group of TP_B = 8 samples
@pytest.mark.parametrize("K", [128, 1024])
def test_text_proj(lib, dev, K, B, N):
    """out[b, n] = bias[n] + sum_k SiLU(text[b, k]) W[n, k].  Chain: K / 64 fma per lane, the butterfly, the bias: n = K / 64 + 7, plus the
    SiLU term of the module docstring."""
    g = torch.Generator(dev).manual_seed(K + 11 * B + N)
    text, W, bias = _rand((B, K), g, dev, 2.0), _rand((N, K), g, dev, K ** -0.5), _rand((N,), g, dev) + 3.0
    f, df = _silu64(text)
    Wd = W.double()
    want = f @ Wd.T + bias.double()
    bound = df @ Wd.abs().T + (K // 64 + 7) * U32 * (f.abs() @ Wd.abs().T + bias.double().abs())
    buf, view = _out(B, N, N, dev)
    _call(lib, "latte_debug_text_proj", text, W, bias, view, B, N, K)
    _, r = _finish(f"text_proj K{K} B{B} N{N}", buf, view, want, bound)
    print(f"text_proj K{K} B{B} N{N}: worst err / bound {r:.3f}")
    assert _rc(lib, "latte_debug_text_proj", text, W, bias, view, B, N, K - 64) == 1


# ------------------------------------------------------------------------------------------------ gated_split_reduce
def _fma32(a, b, c):
    """fp32 fma(a, b, c) with ONE rounding: the product of two fp32 is exact in fp64; the fp64 sum is rounded to odd (TwoSum tells whether it
    was inexact), which makes the second rounding, to fp32, the rounding of the exact value."""
    p, c = a.double() * b.double(), c.double()
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    bits = s.view(torch.int64)
    nudge = (err != 0) & ((bits & 1) == 0)
    up = (err > 0) == (s > 0)                       # towards larger magnitude
    bits = torch.where(nudge, torch.where(up, bits + 1, bits - 1), bits)
    return bits.view(torch.float64).float()


@pytest.mark.parametrize("N", [4, 132])
@pytest.mark.parametrize("splits", [1, 2, 5])
def test_gated_split_reduce(lib, dev, splits, N):
    """x[m, n] += gate[m // rps, n] ((p_0 + p_1 + ...) + bias[n]), slab stride M N + 8 > M N, M = 21 rows of rps = 7: 693 float4 items
    at N = 132, so the 256-thread stripes cut through samples (7 x 33 = 231 items per sample).  Bound: splits - 1 additions, the bias, the
    product and the final add: e (|gate| (splits + 1) (sum |p_s| + |bias|) + |want|).

    Without a tolerance: the same expression in torch fp32 with the slabs added in slab order.  The kernel has one contractible pair, the
    final x + gate * t, and the compiler fuses it (v_pk_fma_f32 in the gfx950 code object), so the torch side takes that step as one fused
    multiply-add too (_fma32); every other operation is a single fp32 add on both sides."""
    M, rps = 21, 7
    stride = M * N + 8
    g = torch.Generator(dev).manual_seed(splits * 100 + N)
    ws = torch.full((splits * stride,), NAN, device=dev)
    slabs = ws.view(splits, stride)[:, :M * N].view(splits, M, N)
    slabs.copy_(_rand((splits, M, N), g, dev))
    bias, gate_buf = _rand((N,), g, dev), _rand((M // rps, N + 4), g, dev)
    gate = gate_buf[:, :N]
    x0 = _rand((M, N), g, dev)
    grow = gate[torch.arange(M, device=dev) // rps]
    t64 = slabs.double().sum(0) + bias.double()
    want = x0.double() + grow.double() * t64
    bound = U32 * (grow.double().abs() * (splits + 1) * (slabs.double().abs().sum(0) + bias.double().abs()) + want.abs())
    buf = torch.full((PAD + M * N + PAD,), SENT, device=dev)
    view = buf[PAD:PAD + M * N].view(M, N)
    view.copy_(x0)
    _call(lib, "latte_debug_gated_split_reduce", view, ws, splits, stride, bias, gate, N + 4, rps, M, N)
    got, r = _finish(f"gated_split_reduce splits {splits} N{N}", buf, view, want, bound)
    a = slabs[0].clone()
    for s in range(1, splits):
        a = a + slabs[s]
    exact = _fma32(a + bias, grow, x0)
    assert torch.equal(got.view(torch.int32), exact.view(torch.int32)), \
        f"gated_split_reduce splits {splits} N{N}: {int((got != exact).sum())} elements differ from the slab-order fp32 evaluation"
    print(f"gated_split_reduce splits {splits} N{N}: worst err / bound {r:.3f}")
    for bad in (dict(N=N + 2), dict(rps=0), dict(stride=M * N - 4), dict(stride=M * N + 6), dict(splits=0)):
        kw = dict(N=N, rps=rps, stride=stride, splits=splits)
        kw.update(bad)
        assert _rc(lib, "latte_debug_gated_split_reduce", view, ws, kw["splits"], kw["stride"], bias, gate, N + 4, kw["rps"], M, kw["N"]) == 1, bad


# ------------------------------------------------------------------------------------------------ adaln_single, cond_rows, mask_bias
@pytest.mark.parametrize("nblk", [1, 4])
@pytest.mark.parametrize("B", [1, 3])
def test_adaln_single(lib, dev, B, nblk):
    """mod[b, j, :] = tables[j, :] + t6[b, j % 6, :] for the 6 nblk block rows, then head_table[r, :] + temb[b, :]: one fp32 add, so the
    result equals torch's fp32 add bit for bit.  D = 136: rows that are no multiple of the 256-thread stripe."""
    D = 136
    g = torch.Generator(dev).manual_seed(B * 10 + nblk)
    tables, head, t6, temb = _rand((nblk * 6, D), g, dev), _rand((2, D), g, dev), _rand((B, 6, D), g, dev), _rand((B, D), g, dev)
    rows = 6 * nblk + 2
    buf, view = _out(B, rows * D, rows * D, dev)
    _call(lib, "latte_debug_adaln_single", tables, head, t6, temb, view, B, nblk, D)
    want = torch.cat([(tables.view(1, nblk, 6, D) + t6.view(B, 1, 6, D)).reshape(B, nblk * 6 * D),
                      (head[None] + temb[:, None]).reshape(B, 2 * D)], dim=1)
    got, _ = _finish(f"adaln_single B{B} nblk{nblk}", buf, view, want.double(), torch.zeros_like(want, dtype=torch.float64))
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))


@pytest.mark.parametrize("n_steps", [1, 4])
@pytest.mark.parametrize("B", [1, 3])
def test_cond_rows(lib, dev, B, n_steps):
    """out[(i, b), :] = SiLU(temb[i, :] (+ ytab[y[b], :])), with and without the label table, a label repeated within the batch.  Bound: the
    add rounds once, which moves SiLU by at most |SiLU'| e |v| <= 1.1 e |v|, plus the SiLU bound of the module docstring."""
    D = 136
    g = torch.Generator(dev).manual_seed(B + 10 * n_steps)
    temb, ytab = _rand((n_steps, D), g, dev, 2.0), _rand((5, D), g, dev, 2.0)
    y = torch.tensor([3, 3, 1][:B], device=dev, dtype=torch.int64)
    for with_table in (False, True):
        v = temb.double()[:, None, :].expand(n_steps, B, D)
        if with_table:
            v = v + ytab.double()[y][None]
        v = v.reshape(n_steps * B, D)
        want, bound = _silu64(v)
        bound = bound + (1.1 * U32 * v.abs() if with_table else 0.0)
        buf, view = _out(n_steps * B, D, D, dev)
        _call(lib, "latte_debug_cond_rows", temb, ytab if with_table else None, y if with_table else None, view, n_steps, B, D)
        _, r = _finish(f"cond_rows B{B} steps {n_steps} table {with_table}", buf, view, want, bound)
        print(f"cond_rows B{B} steps {n_steps} table {with_table}: worst err / bound {r:.3f}")
    assert _rc(lib, "latte_debug_cond_rows", temb, ytab, None, view, n_steps, B, D) == 1


@pytest.mark.parametrize("n", [1, 255, 2 * 120 + 3])
def test_mask_bias(lib, dev, n):
    """bias = (1 - mask) * -10000: a subtraction and a product, no fused pair; equals torch fp32 bit for bit, also for a soft mask."""
    g = torch.Generator(dev).manual_seed(n)
    mask = (torch.rand(n, generator=g, device=dev) < 0.6).float()
    if n > 4:
        mask[::4] = torch.rand(mask[::4].numel(), generator=g, device=dev)
    buf, view = _out(1, n, n, dev)
    _call(lib, "latte_debug_mask_bias", mask, view, n)
    want = ((1.0 - mask) * -10000.0)[None]
    got, _ = _finish(f"mask_bias n{n}", buf, view, want.double(), torch.zeros_like(want, dtype=torch.float64))
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert _rc(lib, "latte_debug_mask_bias", mask, view, 0) == 1
