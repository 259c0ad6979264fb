"""The training step's gradient WRITERS (csrc/train.hip, csrc/train_fin.hip) one kernel at a time through their C-ABI hooks: the two
split reductions, colsum_half, rows_sum, naive_gemm, embedding_bwd, silu_bwd, stage_finalize, adaln_dc, narrow_outer, narrow_dx and
pack_weights.  Every writer runs in its four modes -- assign or add, plain or "the sum leaves the loss-scaled domain" (scale 2^10 in a
device float) -- against an fp64 reference on the same inputs:

    want = out0 * accumulate + sum / scale

Prefill: NaN in assign mode (a read of `out` shows as a non-finite result), random values of magnitude 1e-3 ... 1e3 in add mode.
Everything around the written range holds a sentinel and must come back unchanged.

The bound is per element and first order: slack 2 x 2^-24 x (chain x sum|terms| / scale + |out0| + |want|), chain = the number of fp32
additions behind one output, read off the kernel and written beside each case (the unscale multiplies by a power of two: exact; the
final add rounds once: |out0| + |want| covers it).  None of the bounds is a measured number; the one exception, silu_bwd's fast
exponential, is described in its test.

One check per writer needs no tolerance: the scale is a power of two, so the run with scale 2^10 on inputs multiplied by 2^10 must equal,
bit for bit, the run without a scale on the original inputs -- in assign AND in add mode (the sum, not the accumulated-into value, leaves
the scaled domain).  Magnitudes are drawn in [1e-3, 1e3] so that nothing under- or overflows (f16 operands: up to 30, so that x 2^10 stays
inside f16's range)."""
import ctypes
import itertools

import pytest
import torch

from latte_amd._lib import check, ptr, stream_ptr
from test_train_kernels import DT, ETA, LATTE_ERR_INVALID, TD, U32, U_OUT, _check_elems, _check_rows

pytestmark = pytest.mark.gpu
NAN = float("nan")
SENT = -7.25          # sentinel around every written range
SCALE = 1024.0        # the loss scale of the unscaling modes
MODES = [(0, 0), (0, 1), (1, 0), (1, 1)]   # (accumulate, scaled)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda")


def _mag(shape, g, dev, lo=-3.0, hi=3.0):
    """fp32 values of either sign, magnitude 10^U(lo, hi) per element."""
    e = torch.rand(shape, generator=g, device=dev, dtype=torch.float64) * (hi - lo) + lo
    sgn = torch.where(torch.rand(shape, generator=g, device=dev) < 0.5, -1.0, 1.0)
    return (10.0 ** e).float() * sgn


def _bits(t):
    return t.contiguous().view(torch.int32)


class Out:
    """One output of a writer: `view` (a torch view of the owned elements) inside `buf` (SENT everywhere else).  kind "grad": written in
    the four modes; "grad_nobit": the same, but its terms are not in the scaled domain (no bit check); "scaled": always assigned, stays
    in the scaled domain."""
    def __init__(self, name, buf, view, kind="grad"):
        self.name, self.buf, self.view, self.kind = name, buf, view, kind


def _padded(shape, dev, pad=8, row_pad=0, offset=0):
    """-> (buf, view): view of `shape` inside a SENT-filled buffer, `offset` floats from its start, rows `row_pad` floats apart."""
    if len(shape) == 1:
        buf = torch.full((offset + shape[0] + pad,), SENT, device=dev)
        return buf, buf[offset:offset + shape[0]]
    rows, cols = shape
    buf = torch.full((rows * (cols + row_pad) + pad,), SENT, device=dev)
    return buf, buf[:rows * (cols + row_pad)].view(rows, cols + row_pad)[:, :cols]


def _run_modes(name, alloc, launch, ref, g, dev, modes=MODES):
    """alloc() -> [Out]; launch(mult, {name: view}, accumulate, scale_tensor_or_None) runs the hook on inputs x mult; ref(mult) ->
    {name: (sum, sum_abs, chain)} in fp64 on the same (multiplied) inputs.  Returns {(accumulate, scaled): {name: result}}."""
    scale_t = torch.tensor([SCALE], device=dev)
    res, out0, kinds = {}, {}, {}
    for acc, scaled in modes:
        outs = alloc()
        kinds.update({o.name: o.kind for o in outs})
        for o in outs:
            if o.kind != "scaled" and acc:
                if o.name not in out0:
                    out0[o.name] = _mag(tuple(o.view.shape), g, dev)
                o.view.copy_(out0[o.name])
            else:
                o.view.fill_(NAN)
        mult = SCALE if scaled else 1.0
        launch(mult, {o.name: o.view for o in outs}, acc, scale_t if scaled else None)
        torch.cuda.synchronize()
        refs = ref(mult)
        res[acc, scaled] = {}
        for o in outs:
            tag = f"{name}.{o.name} [accumulate {acc}, scale {'2^10' if scaled else 'none'}]"
            got = o.view.clone()
            assert bool(torch.isfinite(got).all()), f"{tag}: {int((~torch.isfinite(got)).sum())} owned elements not finite (unwritten, or `out` read in assign mode)"
            o.view.fill_(SENT)
            assert bool((_bits(o.buf) == _bits(torch.tensor([SENT], device=dev))).all()), f"{tag}: wrote outside its range"
            tsum, tabs, chain = refs[o.name]
            if o.kind == "scaled":
                want, bound = tsum, U32 * (chain * tabs + tsum.abs())
            else:
                o0 = out0[o.name].double() if acc else torch.zeros_like(tsum)
                want = o0 + tsum / mult
                bound = U32 * (chain * tabs / mult + o0.abs() + want.abs())
            _check_elems(tag, got, want, bound + 1e-300)
            res[acc, scaled][o.name] = got
    for acc in {a for a, _ in modes}:          # the tolerance-free check
        if (acc, 0) in res and (acc, 1) in res:
            for k, kind in kinds.items():
                a, b = res[acc, 0][k], res[acc, 1][k]
                if kind == "grad":
                    assert torch.equal(_bits(a), _bits(b)), f"{name}.{k} accumulate {acc}: the scaled run differs from the unscaled one"
                elif kind == "scaled":
                    assert torch.equal(_bits(a * SCALE), _bits(b)), f"{name}.{k}: did not stay in the scaled domain"
    return res


# ------------------------------------------------------------------------------------------------ split_reduce
def _split_case(lib, dev, n, splits, stride, offset, g, modes=MODES):
    """chain = splits: a = 0 + p_0 + ... + p_{splits-1} in slab order (both kernels), then x 1 / scale (exact) and the final add."""
    part = torch.full((splits * stride + 4,), NAN, device=dev)
    slabs = part[:splits * stride].view(splits, stride)[:, :n]
    base = _mag((splits, n), g, dev)

    def launch(mult, o, acc, sc):
        slabs.copy_(base * mult)
        check(lib.latte_debug_split_reduce(ptr(part), splits, stride, n, ptr(o["out"]), acc, ptr(sc), stream_ptr()))

    def ref(mult):
        d = base.double() * mult
        return {"out": (d.sum(0), d.abs().sum(0), splits)}
    alloc = lambda: [Out("out", *_padded((n,), dev, offset=offset))]
    return _run_modes(f"split_reduce n{n} splits{splits} stride{stride}", alloc, launch, ref, g, dev, modes)


# n: scalar kernel below 4096 (8, 4092), the 16-byte kernel from 4096 on (4096, 4100, 36864), scalar again for n % 4 != 0 (4098)
@pytest.mark.parametrize("n", [8, 4092, 4096, 4100, 36864, 4098])
@pytest.mark.parametrize("splits", [1, 3, 4, 5, 9])     # below, at and past the four-slab step, with tails of 1 (5, 9) and 3 (3)
def test_split_reduce(lib, dev, n, splits):
    g = torch.Generator(dev).manual_seed(n * 31 + splits)
    for stride in (n, n + 4):
        _split_case(lib, dev, n, splits, stride, 0, g)


# the grid-stride loops: scalar kernel (n % 4 != 0) past 4096 blocks x 256 threads, 16-byte kernel past 8192 blocks x 256 float4
@pytest.mark.parametrize("n", [4096 * 256 + 258, 8192 * 1024 + 4096])
def test_split_reduce_grid_stride(lib, dev, n):
    g = torch.Generator(dev).manual_seed(n)
    for stride in (n, n + 4):
        _split_case(lib, dev, n, 2, stride, 0, g)


@pytest.mark.parametrize("splits", [1, 3, 4, 5, 9])
def test_split_reduce_kernels_agree_bit_for_bit(lib, dev, splits):
    """`out` offset by one float takes the scalar fall-back (all four modes checked there); on the same slabs it must give the 16-byte
    kernel's bits in assign mode without a scale: "the same sum in the same order"."""
    n = 36864
    g = torch.Generator(dev).manual_seed(splits)
    a = _split_case(lib, dev, n, splits, n, 0, g, modes=[(0, 0)])
    g = torch.Generator(dev).manual_seed(splits)
    b = _split_case(lib, dev, n, splits, n, 1, g)
    assert torch.equal(_bits(a[0, 0]["out"]), _bits(b[0, 0]["out"]))


# ------------------------------------------------------------------------------------------------ colsum_half
@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("M", [16, 500, 512, 513, 1040])    # one thread row pass, a partial / full / just-started second chunk, three chunks
def test_colsum_half(lib, dev, M, dt):
    """chain: a thread adds 512 / 16 = 32 rows of its chunk, 16 LDS rows are added, then `chunks` chunk sums by the scalar reduction.
    out == NULL: the chunk sums stay in the workspace (chain 32 + 16), assigned, in the scaled domain."""
    g = torch.Generator(dev).manual_seed(M * 3 + DT[dt])
    chunks = (M + 511) // 512
    for C in (8, 120, 128, 136, 1152, 3456):                 # one lane, a partial / full column block, the next block's first lane, 9 and 27 blocks
        base = _mag((M, C), g, dev, -3.0, 1.47 if dt == "f16" else 3.0).to(TD[dt])     # f16: |x| < 30, x 2^10 < 65504
        x = torch.empty_like(base)

        def launch(mult, o, acc, sc, with_out=True):
            x.copy_((base.float() * mult).to(TD[dt]))
            assert torch.equal(x.float(), base.float() * mult)           # the multiplied operand is exact
            check(lib.latte_debug_colsum_half(ptr(x), M, C, ptr(o["ws"]), chunks * C, ptr(o["out"]) if with_out else None, acc, DT[dt],
                                              ptr(sc), stream_ptr()))

        def ref(mult):
            d = base.double() * mult
            pad = torch.zeros(chunks * 512 - M, C, device=dev, dtype=torch.float64)
            ch = torch.cat([d, pad]).view(chunks, 512, C)
            return {"out": (d.sum(0), d.abs().sum(0), 32 + 16 + chunks), "ws": (ch.sum(1), ch.abs().sum(1), 32 + 16)}
        alloc = lambda: [Out("out", *_padded((C,), dev)), Out("ws", *_padded((chunks, C), dev), kind="scaled")]
        _run_modes(f"colsum_half M{M} C{C} {dt}", alloc, launch, ref, g, dev)
        alloc = lambda: [Out("ws", *_padded((chunks, C), dev), kind="scaled")]
        _run_modes(f"colsum_half(out NULL) M{M} C{C} {dt}", alloc, lambda m, o, a, s: launch(m, o, a, s, False), ref, g, dev,
                   modes=[(0, 0), (0, 1)])


def test_colsum_half_refuses_a_width_it_cannot_take(lib, dev):
    x = torch.ones(16, 12, device=dev, dtype=torch.float16)
    ws = torch.full((64,), SENT, device=dev)
    out = torch.full((64,), SENT, device=dev)
    rc = lib.latte_debug_colsum_half(ptr(x), 16, 12, ptr(ws), 64, ptr(out), 0, 1, None, stream_ptr())
    torch.cuda.synchronize()
    assert rc == LATTE_ERR_INVALID and bool((ws == SENT).all()) and bool((out == SENT).all())


# ------------------------------------------------------------------------------------------------ rows_sum
@pytest.mark.parametrize("B", [1, 9])
@pytest.mark.parametrize("N", [255, 256, 257, 6912])       # a partial block, a full one, one column into the second, 27 blocks
def test_rows_sum(lib, dev, N, B):
    """chain = B: one thread per column adds the B rows in order."""
    g = torch.Generator(dev).manual_seed(N * 11 + B)
    for stride in (N, N + 64):
        base = _mag((B, N), g, dev)
        src = torch.full((B, stride), NAN, device=dev)

        def launch(mult, o, acc, sc):
            src[:, :N] = base * mult
            check(lib.latte_debug_rows_sum(ptr(src), B, stride, N, ptr(o["out"]), acc, ptr(sc), stream_ptr()))

        def ref(mult):
            d = base.double() * mult
            return {"out": (d.sum(0), d.abs().sum(0), B)}
        _run_modes(f"rows_sum B{B} N{N} stride{stride}", lambda: [Out("out", *_padded((N,), dev))], launch, ref, g, dev)


# ------------------------------------------------------------------------------------------------ naive_gemm
def _gemm_case(lib, dev, name, g, M, N, K, splits, a_store, a_mat, a_strides, b_store, b_mat, b_strides, scale_a):
    """a_mat / b_mat: functions of the stored tensor -> the [M, K] / [K, N] matrix it represents.
    chain: a K range of kc elements runs four chains of kc / 4 products (+ up to 3 tail products on the first), two levels combine
    them, each product and alpha round once (no more with an FMA): ceil(kc / 4) + 3 + 2 + 2; the reduction adds the ns partial products."""
    kc = (K + splits - 1) // splits
    ns = (K + kc - 1) // kc
    chain = (kc + 3) // 4 + 3 + 2 + 2 + (ns if splits > 1 else 0)
    ws = torch.full((max(splits * M * N, 1) + 4,), NAN, device=dev)
    a_dev, b_dev = a_store.clone(), b_store.clone()

    def launch(mult, o, acc, sc):
        a_dev.copy_(a_store * (mult if scale_a else 1.0))
        b_dev.copy_(b_store * (1.0 if scale_a else mult))
        check(lib.latte_debug_naive_gemm(ptr(a_dev), a_strides[0], a_strides[1], ptr(b_dev), b_strides[0], b_strides[1], ptr(o["C"]), N, 1,
                                         M, N, K, 1.0, acc, splits, ptr(ws) if splits > 1 else None, splits * M * N, ptr(sc), stream_ptr()))

    def ref(mult):
        a = torch.nan_to_num(a_mat(a_store)).double() * (mult if scale_a else 1.0)
        b = torch.nan_to_num(b_mat(b_store)).double() * (1.0 if scale_a else mult)
        return {"C": (a @ b, a.abs() @ b.abs(), chain)}
    _run_modes(name, lambda: [Out("C", *_padded((M, N), dev))], launch, ref, g, dev)


@pytest.mark.parametrize("N", [8, 32, 1152])
@pytest.mark.parametrize("K", [40, 64, 1000])     # fewer rows than splits (40 one-row ranges), one row per split, 16-row ranges with a short last one
def test_naive_gemm_bias_sum(lib, dev, N, K):
    """The trainer's bias gradient of a narrow linear: ones[K] (row stride 0) x dY[K, N], 64 splits."""
    g = torch.Generator(dev).manual_seed(N * 7 + K)
    ones = torch.ones(K, device=dev)
    dy = _mag((K, N), g, dev)
    _gemm_case(lib, dev, f"naive_gemm bias N{N} K{K}", g, 1, N, K, 64, ones, lambda s: s[None, :], (0, 1), dy, lambda s: s, (N, 1), False)


@pytest.mark.parametrize("B", [1, 3, 5])          # K = batch: only the tail loop below 4, one unrolled step + tail at 5
@pytest.mark.parametrize("D,M", [(128, 6), (1152, 7), (63, 6), (65, 7)])   # N = 63 / 65: a partial block, one column into the second
def test_naive_gemm_outer_product(lib, dev, B, D, M):
    """dW[n, k] = sum_b dmod[b, n] csilu[b, k]: A is read transposed out of [B, nmod] rows (sam = 1, sak = nmod), one launch."""
    g = torch.Generator(dev).manual_seed(B * 13 + D + M)
    nmod = M + 5
    dm = torch.full((B, nmod), NAN, device=dev)
    dm[:, :M] = _mag((B, M), g, dev)
    cs = _mag((B, D), g, dev, -2.0, 1.0)
    _gemm_case(lib, dev, f"naive_gemm outer B{B} D{D} M{M}", g, M, D, B, 1, dm, lambda s: s[:, :M].t(), (1, nmod), cs, lambda s: s, (D, 1), True)


@pytest.mark.parametrize("B", [3, 9])             # a partial block row, three block rows
def test_naive_gemm_split_48(lib, dev, B):
    """d silu(c) = dmod[B, 6912] W[6912, 128] on 48 ranges of 144 rows, reduced into the output (assign in the trainer; add as well here)."""
    g = torch.Generator(dev).manual_seed(B)
    K, N = 6912, 128
    a = _mag((B, K), g, dev)
    w = _mag((K, N), g, dev, -2.0, 0.0)
    _gemm_case(lib, dev, f"naive_gemm split48 B{B}", g, B, N, K, 48, a, lambda s: s, (K, 1), w, lambda s: s, (N, 1), True)


def test_naive_gemm_refuses_a_split_launch_with_a_strided_output(lib, dev):
    a = torch.ones(4, 64, device=dev)
    b = torch.ones(64, 8, device=dev)
    c = torch.full((4 * 16,), SENT, device=dev)
    ws = torch.full((4 * 4 * 8,), SENT, device=dev)
    rc = lib.latte_debug_naive_gemm(ptr(a), 64, 1, ptr(b), 8, 1, ptr(c), 16, 1, 4, 8, 64, 1.0, 0, 4, ptr(ws), ws.numel(), None, stream_ptr())
    torch.cuda.synchronize()
    assert rc == LATTE_ERR_INVALID and bool((c == SENT).all()) and bool((ws == SENT).all())


# ------------------------------------------------------------------------------------------------ embedding_bwd
@pytest.mark.parametrize("D", [128, 257, 1152])   # half a block, one column into the second, 4.5 blocks
def test_embedding_bwd(lib, dev, D):
    """dtable[idx[b]] += dc[b] / scale, b in order; always adds, so the table is prefilled.  Label 2 twice, labels 1, 4, 6 never: their
    rows must come back bit for bit.  chain = the number of samples that carry the row's label."""
    g = torch.Generator(dev).manual_seed(D)
    idx = torch.tensor([2, 0, 2, 5, 3], device=dev)
    B, rows = 5, 7
    dc = _mag((B, D), g, dev)
    t0 = _mag((rows, D), g, dev)
    onehot = torch.zeros(rows, B, device=dev, dtype=torch.float64)
    onehot[idx, torch.arange(B, device=dev)] = 1.0
    got = {}
    for scaled in (0, 1):
        mult = SCALE if scaled else 1.0
        buf = torch.full((rows * D + 8,), SENT, device=dev)
        tab = buf[:rows * D].view(rows, D)
        tab.copy_(t0)
        src = dc * mult
        sc = torch.tensor([SCALE], device=dev) if scaled else None
        check(lib.latte_debug_embedding_bwd(ptr(src), ptr(idx), ptr(tab), B, D, ptr(sc), stream_ptr()))
        torch.cuda.synchronize()
        tsum, tabs = onehot @ dc.double(), onehot @ dc.double().abs()
        want = t0.double() + tsum
        cnt = onehot.sum(1, keepdim=True)
        _check_elems(f"embedding_bwd D{D} scaled{scaled}", tab, want, U32 * (cnt * tabs + t0.double().abs() + want.abs()))
        for r in (1, 4, 6):
            assert torch.equal(_bits(tab[r]), _bits(t0[r])), r
        assert bool((buf[rows * D:] == SENT).all())
        got[scaled] = tab.clone()
    assert torch.equal(_bits(got[0]), _bits(got[1]))


# ------------------------------------------------------------------------------------------------ silu_bwd
def _silu_grad64(x):
    s = 1.0 / (1.0 + torch.exp(-x))
    return s * (1.0 + x * (1.0 - s))


@pytest.mark.parametrize("n", [1, 255, 257, 9 * 1152])
def test_silu_bwd(lib, dev, n):
    """din (+)= dout * s (1 + x (1 - s)), s = 1 / (1 + __expf(-x)), x in [-20, 20] with 0 among them; separate and in place (din == dout,
    as the trainer runs the timestep MLP's backward).

    Bound: 8 fp32 operations (negate, exp argument, add, divide, subtract, two multiplies and an add, the product with dout), each
    relative to a term no larger than |v| (1 + |x|), v = dout silu'(x): 8 x 2^-24 x |v| (1 + |x|); plus the error of the fast exponential
    and of the cancellation in 1 - s beside it.  The ROCm device-library documentation installed with the toolchain states no error
    figure for __expf, so that part is taken, as an absolute error of the silu' factor, from the fp32 CPU evaluation of the same
    expression against fp64 over this test's inputs -- 9.8e-7 at the worst input of the 9 x 1152 grid (the cancellation in 1 - s near
    x = 5), recomputed here on the very inputs -- and 4 x that, times |dout|, is allowed.  Add mode: one more rounding, |din0| + |want|."""
    g = torch.Generator(dev).manual_seed(17)
    x_all = torch.rand(9 * 1152, generator=g, device=dev) * 40 - 20        # every case reads a prefix of the largest case's inputs
    x_all[::7] = torch.linspace(-20, 20, x_all[::7].numel(), device=dev)
    x_all[0] = 0.0
    xc = x_all.cpu()
    s32 = 1.0 / (1.0 + torch.exp(-xc))
    f32 = s32 * (1.0 + xc * (1.0 - s32))
    e_fast = 4.0 * float((f32.double() - _silu_grad64(xc.double())).abs().max())
    print(f"silu_bwd: fp32 CPU error of the silu' factor over the inputs {e_fast / 4:.3e}")
    assert 0.0 < e_fast < 8e-6
    x = x_all[:n].clone()
    dout = _mag((n,), g, dev)
    xd = x.double()
    fd = _silu_grad64(xd)
    v = dout.double() * fd
    base_bound = 8 * U32 * v.abs() * (1 + xd.abs()) + e_fast * dout.double().abs()
    for acc in (0, 1):
        d0 = _mag((n,), g, dev)
        buf, din = _padded((n,), dev)
        din.copy_(d0) if acc else din.fill_(NAN)
        check(lib.latte_debug_silu_bwd(ptr(dout), ptr(x), ptr(din), n, acc, stream_ptr()))
        torch.cuda.synchronize()
        want = v + (d0.double() if acc else 0.0)
        assert bool(torch.isfinite(din).all())
        _check_elems(f"silu_bwd n{n} acc{acc} separate", din, want, base_bound + acc * U32 * (d0.double().abs() + want.abs()), slack=1.0)
        sep = din.clone()
        din.fill_(SENT)
        assert bool((buf == SENT).all())
        if not acc:                                   # in place: din == dout (accumulating in place would read dout as din: not a trainer form)
            buf, io = _padded((n,), dev)
            io.copy_(dout)
            check(lib.latte_debug_silu_bwd(ptr(io), ptr(x), ptr(io), n, 0, stream_ptr()))
            torch.cuda.synchronize()
            assert torch.equal(_bits(io), _bits(sep))
            io.fill_(SENT)
            assert bool((buf == SENT).all())


# ------------------------------------------------------------------------------------------------ stage_finalize
def _arr(ctype, vals):
    return (ctype * max(len(vals), 1))(*vals)


def _ptr_arr(tensors):
    return _arr(ctypes.c_void_p, [t.data_ptr() for t in tensors])


# (D, B, partial rows per sample, n_mod, [(bias_rows, bias_cols: "D" | "3D" | "4D" | 200)]): the two extremes of every axis, every
# bias_rows value once: 1 / 15 / 16 / 17 = below, at and past one pass of the 16 thread rows; 49 = the first four-chain step
# (r + 48 < rows for r = 0 only); 63 / 64 / 65 around it for every thread row; 130 = two steps and a tail.  B = 9 / 17: a second and a
# third pass over samples, which read, modify and write db and dW.
FIN_CASES = [
    (64, 1, 2, 2, [(1, "D")]),
    (128, 8, 16, 6, [(15, "D"), (16, "3D"), (17, "4D"), (49, 200)]),
    (1152, 9, 17, 6, [(63, "D"), (64, "3D"), (65, "4D"), (130, 200)]),
    (1280, 17, 128, 6, []),
    (1280, 17, 2, 0, [(130, "4D"), (1, 200), (64, "D"), (16, "3D")]),
    (64, 17, 128, 2, []),
]


@pytest.mark.parametrize("D,B,prs,n_mod,biases", FIN_CASES, ids=[f"D{c[0]}-B{c[1]}-rows{c[2]}-mod{c[3]}-bias{len(c[4])}" for c in FIN_CASES])
def test_stage_finalize(lib, dev, D, B, prs, n_mod, biases):
    """chains: dmod[b][col] = 16 thread rows of ceil(prs / 16) partial rows each, then 16 LDS adds: cm = ceil(prs / 16) + 16;
    db = dmod's chain + the B samples + one add per pass of 8; dW = dmod's chain + B fused multiply-adds + one add per pass;
    a bias sum = ceil(rows / 16) rows per thread row on four chains (2 adds to combine) + 16 LDS adds."""
    g = torch.Generator(dev).manual_seed(D * 3 + B * 5 + prs)
    nsum = [1 + c % 2 for c in range(n_mod)]
    which = [(c // 2) % nsum[c] for c in range(n_mod)]                      # 0, 0, 0, 1, 0, 0 with nsum 1, 2, 1, 2, 1, 2
    base_mod = [_mag((B, prs, D), g, dev) for _ in range(n_mod)]
    mod_src = [torch.full((B * prs, nsum[c], D), NAN, device=dev) for c in range(n_mod)]
    csilu = _mag((B, D), g, dev, -2.0, 1.0)
    cols = {"D": D, "3D": 3 * D, "4D": 4 * D, 200: 200}
    bias = [(r, cols[c], cols[c] + 24) for r, c in biases]                  # rows, cols, stride > cols
    base_bias = [_mag((r, c), g, dev) for r, c, _ in bias]
    bias_src = [torch.full((r, s), NAN, device=dev) for r, _, s in bias]
    dstride = n_mod * D + 24
    passes = (B + 7) // 8
    cm = (prs + 15) // 16 + 16

    def alloc():
        outs = []
        if n_mod:
            outs += [Out("dmod", *_padded((B, n_mod * D), dev, row_pad=24), kind="scaled"), Out("db", *_padded((n_mod * D,), dev)),
                     Out("dW", *_padded((n_mod * D * D,), dev))]
        return outs + [Out(f"bias{i}", *_padded((c,), dev, pad=s - c)) for i, (_, c, s) in enumerate(bias)]

    def launch(mult, o, acc, sc):
        for c in range(n_mod):
            mod_src[c][:, which[c], :] = (base_mod[c] * mult).view(B * prs, D)
        for i, (_, c, _) in enumerate(bias):
            bias_src[i][:, :c] = base_bias[i] * mult
        d = torch.zeros(1, device=dev)
        bout = [o[f"bias{i}"] for i in range(len(bias))]
        check(lib.latte_debug_stage_finalize(
            _ptr_arr(mod_src), _arr(ctypes.c_int, nsum), _arr(ctypes.c_int, which), n_mod, prs, B, D, ptr(o.get("dmod", d)), dstride,
            ptr(csilu), ptr(o.get("dW", d)), ptr(o.get("db", d)), len(bias), _ptr_arr(bias_src), _arr(ctypes.c_int, [b[0] for b in bias]),
            _arr(ctypes.c_int, [b[2] for b in bias]), _arr(ctypes.c_int, [b[1] for b in bias]), _ptr_arr(bout), ptr(sc), acc, stream_ptr()))

    def ref(mult):
        r = {}
        if n_mod:
            part = torch.stack(base_mod, 1).double() * mult                  # [B, n_mod, prs, D]
            dm, dma = part.sum(2).view(B, n_mod * D), part.abs().sum(2).view(B, n_mod * D)
            cd = csilu.double()
            r["dmod"] = (dm, dma, cm)
            r["db"] = (dm.sum(0), dma.sum(0), cm + B + passes)
            r["dW"] = ((dm.t() @ cd).reshape(-1), (dma.t() @ cd.abs()).reshape(-1), cm + B + passes + 1)
        for i, (rows, _, _) in enumerate(bias):
            d = base_bias[i].double() * mult
            r[f"bias{i}"] = (d.sum(0), d.abs().sum(0), (rows + 15) // 16 + 2 + 16)
        return r
    _run_modes(f"stage_finalize D{D} B{B}", alloc, launch, ref, g, dev)


@pytest.mark.parametrize("D,n_mod", [(96, 2), (128, 7)])
def test_stage_finalize_refuses(lib, dev, D, n_mod):
    B, prs = 2, 2
    src = [torch.ones(B * prs, 1, D, device=dev) for _ in range(n_mod)]
    outs = [torch.full(s, SENT, device=dev) for s in ((B, n_mod * D), (n_mod * D, D), (n_mod * D,), (D,))]
    cs = torch.ones(B, D, device=dev)
    rc = lib.latte_debug_stage_finalize(_ptr_arr(src), _arr(ctypes.c_int, [1] * n_mod), _arr(ctypes.c_int, [0] * n_mod), n_mod, prs, B, D,
                                        ptr(outs[0]), n_mod * D, ptr(cs), ptr(outs[1]), ptr(outs[2]), 1, _ptr_arr([src[0]]),
                                        _arr(ctypes.c_int, [B * prs]), _arr(ctypes.c_int, [D]), _arr(ctypes.c_int, [D]), _ptr_arr([outs[3]]),
                                        None, 0, stream_ptr())
    torch.cuda.synchronize()
    assert rc == LATTE_ERR_INVALID and all(bool((o == SENT).all()) for o in outs)


# ------------------------------------------------------------------------------------------------ adaln_dc
# nmod = depth * 6 D + 2 D: 512 (one partial split), 1792 (a block boundary inside split 0 and 1), 21760 (22 splits, the last a quarter
# full, boundaries at every offset), 16128 (15.75 splits at the widest rows)
@pytest.mark.parametrize("depth,D", [(1, 64), (2, 128), (28, 128), (2, 1152)])
@pytest.mark.parametrize("B", [1, 8, 9])            # 9: a second pass over samples
def test_adaln_dc(lib, dev, depth, D, B):
    """dc = dmod [B, nmod] x the concatenated adaLN weight rows [nmod, D] (fp64 matmul).  The weights sit in a flat buffer with other
    tensors between them (NaN here).  chain: 1024 / 16 = 64 fused multiply-adds per thread row, 16 LDS adds, the splits."""
    g = torch.Generator(dev).manual_seed(depth * 100 + D + B)
    rows6 = 6 * D
    nmod = depth * rows6 + 2 * D
    splits = (nmod + 1023) // 1024
    stride = rows6 * D + 2 * D + 4
    flat = torch.full((depth * stride,), NAN, device=dev)
    wb = flat.view(depth, stride)[:, :rows6 * D]
    wb.copy_(_mag((depth, rows6 * D), g, dev, -3.0, 0.0))
    wf = _mag((2 * D, D), g, dev, -3.0, 0.0)
    dmod = _mag((B, nmod), g, dev)
    W = torch.cat([wb.reshape(depth * rows6, D), wf]).double()
    ws = torch.full((splits * B * D + 4,), SENT, device=dev)

    def launch(mult, o, acc, sc):
        check(lib.latte_debug_adaln_dc(ptr(dmod), nmod, B, ptr(flat), stride, depth, rows6, ptr(wf), D, ptr(ws), splits * B * D, ptr(o["dc"]),
                                       stream_ptr()))
    ref = lambda mult: {"dc": ((dmod.double() @ W).reshape(-1), (dmod.double().abs() @ W.abs()).reshape(-1), 64 + 16 + splits)}
    _run_modes(f"adaln_dc depth{depth} D{D} B{B}", lambda: [Out("dc", *_padded((B * D,), dev), kind="scaled")], launch, ref, g, dev,
               modes=[(0, 0)])
    assert bool((ws[splits * B * D:] == SENT).all())


# ------------------------------------------------------------------------------------------------ narrow_outer / narrow_dx
NO_P = [1, 8, 12, 16, 32]            # one column, P % 4 == 0 and not (12 % 8), the 32 bound
NO_D = [128, 260, 1152, 1280]        # D / 4 = 32 (half a wave), 65 (a second wave with one lane), 288 (4.5 waves), 320 (the bound)
NO_M = [16, 100, 128, 129, 1000]     # one LDS stage, a partial stage, one full block, one row into the second, 8 blocks with a partial last


def _pairwise(axes):
    """A deterministic greedy covering array: every pair of values of every two axes occurs in some case."""
    todo = {(i, a, j, b) for i, j in itertools.combinations(range(len(axes)), 2) for a in axes[i] for b in axes[j]}
    full = list(itertools.product(*axes))
    cases = []
    while todo:
        cover = lambda c: sum((i, c[i], j, c[j]) in todo for i, j in itertools.combinations(range(len(axes)), 2))
        best = max(full, key=cover)
        cases.append(best)
        todo -= {(i, best[i], j, best[j]) for i, j in itertools.combinations(range(len(axes)), 2)}
    return cases


NO_CASES = _pairwise([NO_P, NO_D, NO_M, ["f32", "bf16", "f16"], [0, 1], [0, 1], [0, 1]])


@pytest.mark.parametrize("P,D,M,wide,layout,with_nsum,with_wsum", NO_CASES, ids=["-".join(str(v) for v in c) for c in NO_CASES])
def test_narrow_outer(lib, dev, P, D, M, wide, layout, with_nsum, with_wsum):
    """dW[p][k] (layout 0: (so_p, so_k) = (D, 1); 1: (1, P)) = sum_m nar[m][p] wide[m][k], with the column sums of either operand.  The
    narrow operand carries the loss scale here (the final linear's form); the wide operand's column sum is then outside the bit check.
    chain: a block adds its 128 rows by fused multiply-adds (plain adds for the column sums), the reduction the ceil(M / 128) blocks."""
    g = torch.Generator(dev).manual_seed(P * 1000 + D + M)
    nb = (M + 127) // 128
    nar0 = _mag((M, P), g, dev)
    nar = torch.empty_like(nar0)
    wd = _mag((M, D), g, dev, -3.0, 2.0)
    if wide != "f32":
        wd = wd.to(TD[wide])
    so = (D, 1) if layout == 0 else (1, P)
    ws_floats = nb * (P * D + P + D)
    ws = torch.full((ws_floats + 4,), SENT, device=dev)

    def alloc():
        outs = [Out("dW", *_padded((P * D,), dev))]
        if with_nsum:
            outs.append(Out("nsum", *_padded((P,), dev)))
        if with_wsum:
            outs.append(Out("wsum", *_padded((D,), dev), kind="grad_nobit"))
        return outs

    def launch(mult, o, acc, sc):
        nar.copy_(nar0 * mult)
        check(lib.latte_debug_narrow_outer(ptr(nar), P, ptr(wd), int(wide != "f32"), D, M, ptr(o["dW"]), so[0], so[1], ptr(o.get("nsum")),
                                           ptr(o.get("wsum")), ptr(ws), ws_floats, DT.get(wide, 1), ptr(sc), acc, stream_ptr()))

    def ref(mult):
        a, w = nar0.double() * mult, wd.double()
        pk, pka = a.t() @ w, a.abs().t() @ w.abs()                          # [P, D]
        if layout == 1:
            pk, pka = pk.t(), pka.t()
        return {"dW": (pk.reshape(-1), pka.reshape(-1), 128 + nb), "nsum": (a.sum(0), a.abs().sum(0), 128 + nb),
                "wsum": (w.sum(0), w.abs().sum(0), 128 + nb)}
    _run_modes(f"narrow_outer P{P} D{D} M{M} {wide}", alloc, launch, ref, g, dev)
    assert bool((ws[ws_floats:] == SENT).all())


DX_CASES = [(P, D, NO_M[(i + j) % 5], ("bf16", "f16")[(i + j) % 2]) for i, P in enumerate(NO_P) for j, D in enumerate(NO_D)]
DX_CASES += [(P, D, M, "f16" if dt == "bf16" else "bf16") for P, D, M, dt in DX_CASES[::3]]


@pytest.mark.parametrize("P,D,M,dt", DX_CASES, ids=["-".join(str(v) for v in c) for c in DX_CASES])
def test_narrow_dx(lib, dev, P, D, M, dt):
    """out[m][k] = half(sum_p nar[m][p] W[p][k]): bound u_out |want| + P x 2^-24 sum|terms| (P fused multiply-adds; f16: + the subnormal step)."""
    g = torch.Generator(dev).manual_seed(P * 1000 + D + M)
    nar = _mag((M, P), g, dev, -3.0, 1.0)
    W = torch.randn(P, D, generator=g, device=dev)
    buf = torch.full((M * D + 8,), SENT, device=dev, dtype=TD[dt])
    out = buf[:M * D].view(M, D)
    out.fill_(NAN)
    check(lib.latte_debug_narrow_dx(ptr(nar), P, ptr(W), D, M, ptr(out), DT[dt], stream_ptr()))
    torch.cuda.synchronize()
    want = nar.double() @ W.double()
    assert bool(torch.isfinite(out).all())
    # (_check_elems' slack of 2, as everywhere in test_train_kernels.py: U_OUT["bf16"] = 2^-9 is half of bf16's unit roundoff 2^-8)
    _check_elems(f"narrow_dx P{P} D{D} M{M} {dt}", out, want, U_OUT[dt] * want.abs() + ETA[dt] + P * U32 * (nar.double().abs() @ W.double().abs()))
    assert bool((buf[M * D:] == SENT).all())


@pytest.mark.parametrize("P,D", [(33, 128), (8, 1284), (8, 130)])
def test_narrow_kernels_refuse(lib, dev, P, D):
    M = 16
    nar = torch.ones(M, P, device=dev)
    wd = torch.ones(M, D, device=dev)
    W = torch.ones(P, D, device=dev)
    outs = [torch.full((n,), SENT, device=dev) for n in (P * D, P, D, P * D + P + D)]
    hout = torch.full((M * D,), SENT, device=dev, dtype=torch.float16)
    rc = lib.latte_debug_narrow_outer(ptr(nar), P, ptr(wd), 0, D, M, ptr(outs[0]), D, 1, ptr(outs[1]), ptr(outs[2]), ptr(outs[3]),
                                      outs[3].numel(), 1, None, 0, stream_ptr())
    rc2 = lib.latte_debug_narrow_dx(ptr(nar), P, ptr(W), D, M, ptr(hout), 1, stream_ptr())
    torch.cuda.synchronize()
    assert rc == LATTE_ERR_INVALID and rc2 == LATTE_ERR_INVALID
    assert all(bool((o == SENT).all()) for o in outs) and bool((hout == SENT).all())


# ------------------------------------------------------------------------------------------------ pack_weights
@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("D,blocks", [(72, 3), (128, 1)])      # 72: N and K no multiples of the 32 x 32 tile
def test_pack_weights(lib, dev, D, blocks, dt):
    """The one-launch pack of every block weight against the per-matrix kernel (bit for bit) and against w.to(dtype) / w.t().to(dtype)."""
    g = torch.Generator(dev).manual_seed(D)
    shapes = [(3 * D, D), (D, D), (4 * D, D), (D, 4 * D)]
    w, bufs, views = [], [], []
    for _ in range(blocks):
        for N, K in shapes:
            w.append(_mag((N, K), g, dev, -3.0, 1.0))
            b = [torch.full((N * K + 8,), SENT, device=dev, dtype=TD[dt]) for _ in range(2)]
            bufs.append(b)
            views.append((b[0][:N * K].view(N, K), b[1][:N * K].view(K, N)))
    check(lib.latte_debug_pack_weights(_ptr_arr(w), _arr(ctypes.c_int, [s[0] for s in shapes]), _arr(ctypes.c_int, [s[1] for s in shapes]),
                                       _ptr_arr([v[0] for v in views]), _ptr_arr([v[1] for v in views]), blocks, DT[dt], stream_ptr()))
    torch.cuda.synchronize()
    for i, wi in enumerate(w):
        N, K = wi.shape
        one = [torch.empty(N, K, device=dev, dtype=TD[dt]), torch.empty(K, N, device=dev, dtype=TD[dt])]
        check(lib.latte_debug_pack_weight(ptr(wi), ptr(one[0]), ptr(one[1]), N, K, DT[dt], stream_ptr()))
        torch.cuda.synchronize()
        wn, wt = views[i]
        i16 = lambda t: t.contiguous().view(torch.int16)
        assert torch.equal(i16(wn), i16(one[0])) and torch.equal(i16(wt), i16(one[1])), i
        assert torch.equal(i16(wn), i16(wi.to(TD[dt]))) and torch.equal(i16(wt), i16(wi.t().contiguous().to(TD[dt]))), i
        assert all(bool((b[N * K:] == SENT).all()) for b in bufs[i]), i
