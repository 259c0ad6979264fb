"""The LoRA kernels of csrc/train_lora.hip through their C-ABI hooks: the row-local product (h = s x A^T, g = s dY B), the chunked outer
product + fixed-order reduction (dA, dB) and the merged weight pack, each against an fp64 CPU reference on inputs rounded to the
operand type first, compared per element.

The row-local product writes a split pair [hi | lo]: hi = half(v), lo = half((v - hi) L) with L = 2048 (f16) / 256 (bf16), and the outer
product contracts hi + lo / L.

Bounds (derived, none measured): a half output is one rounding of an fp32 sum, u |ref| + n 2^-24 sum|terms| with u the unit roundoff of
the operand type and n the contraction length (products of two halves are exact in fp32, so the only fp32 errors are the n additions and
the scale) -- that is hi's bound; the pair hi + lo / L leaves u^2 |ref| + 2^-24 / L (lo's rounding: relative u of a remainder of at
most u |ref|, or f16's subnormal step 2^-24 where the remainder is that small) on top of the fp32 sum's n 2^-24 sum|terms|;
an fp32 output is n 2^-24 sum|terms| -- with n the number of fp32 roundings behind an element, which is the contraction length plus
the few more named at each bound (the outer product: M additions, + 1 for lo's product by 1 / L, + 1 for joining the two accumulators,
+ 1 for adding into the gradient buffer in accumulate mode; the merge: r fma of the sum, + 1 for s times the sum plus W, + 1 for
the reference's own fp32 rounding of B and A products being compared in fp64); the pack is within one ulp of the operand type of torch's fp32 W + s B A (the two fp32
sums differ by their own rounding, which can move the half rounding by one step), and with B = 0 it is the plain pack bit for bit."""
import ctypes

import pytest
import torch

from latte_amd._lib import check, ptr, stream_ptr

pytestmark = pytest.mark.gpu
TD = {"bf16": torch.bfloat16, "f16": torch.float16}
DT = {"bf16": 0, "f16": 1}
U = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11}
U32 = 2.0 ** -24
LO = {"bf16": 256.0, "f16": 2048.0}
SENT = -77.0
MS = [64, 192, 320]            # one chunk, several chunks, a last partial chunk (the trainer guarantees M % 64 == 0)
KS = [128, 384, 512, 1152]     # 1, 3, 4 and 9 chunks of 128 columns over the down kernel's four waves
CHUNK = {64: 64, 192: 64, 320: 128}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda")


def r16(r):
    return (r + 15) // 16 * 16


def half_randn(shape, g, dt, scale=1.0):
    """N(0, scale) rounded to the operand type -> (the half tensor on the CPU, its exact fp64 value)."""
    h = (torch.randn(shape, generator=g) * scale).to(TD[dt])
    return h, h.double()


def check_elems(label, got, want, bound):
    err = (got.double().cpu() - want).abs()
    bad = err > bound
    assert not bool(bad.any()), (label, int(bad.sum()), float((err / bound.clamp_min(1e-300)).max()))


@pytest.mark.parametrize("r", [4, 16, 64])
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_down(lib, dev, dt, r):
    """out [M, 2 R16] = [hi | lo] of scale big [M, Kbig] wd [R16, Kbig]^T, the padding columns exactly zero, nothing written behind it."""
    g = torch.Generator().manual_seed(100 + r)
    R, scale = r16(r), 1.5
    for M in MS:
        for K in KS:
            big, big64 = half_randn((M, K), g, dt)
            wd, wd64 = half_randn((r, K), g, dt, K ** -0.5)
            wd_pad = torch.zeros(R, K, dtype=TD[dt])
            wd_pad[:r] = wd
            buf = torch.full((M * 2 * R + 64,), SENT, dtype=TD[dt], device=dev)
            big_d, wd_d = big.to(dev), wd_pad.to(dev)
            check(lib.latte_debug_lora_down(ptr(big_d), ptr(wd_d), ptr(buf), M, K, r, scale, DT[dt], stream_ptr()))
            torch.cuda.synchronize()
            out = buf[:M * 2 * R].view(M, 2 * R)
            hi, lo = out[:, :R], out[:, R:]
            want = scale * big64 @ wd64.T
            terms = scale * big64.abs() @ wd64.abs().T
            check_elems(f"down hi {dt} r{r} M{M} K{K}", hi[:, :r], want, U[dt] * want.abs() + K * U32 * terms)
            check_elems(f"down pair {dt} r{r} M{M} K{K}", hi[:, :r].double() + lo[:, :r].double() / LO[dt], want,
                        U[dt] ** 2 * want.abs() + U32 / LO[dt] + (K + 2) * U32 * terms)
            assert float(torch.cat([hi[:, r:], lo[:, r:]]).float().abs().max() if R > r else 0.0) == 0.0
            assert bool((buf[M * 2 * R:] == SENT).all())


@pytest.mark.parametrize("kr", [0, 1])
@pytest.mark.parametrize("r", [4, 16, 64])
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_outer(lib, dev, dt, r, kr):
    """sum_m (hi + lo / L)[m, :r] (x) big[m, :] in dA's layout [r, Kbig] (kr = 0) and dB's [Kbig, r] (kr = 1); the padding columns of hi
    and lo hold garbage here and must reach nothing."""
    g = torch.Generator().manual_seed(200 + r + kr)
    R = r16(r)
    for M in MS:
        for K in KS:
            small, small64 = half_randn((M, 2 * R), g, dt)
            small64 = small64[:, :R] + small64[:, R:] / LO[dt]             # what the pair stands for
            big, big64 = half_randn((M, K), g, dt)
            chunk = CHUNK[M]
            chunks = -(-M // chunk)
            ws = torch.full((chunks * r * K + 32,), SENT, device=dev)
            buf = torch.full((r * K + 32,), SENT, device=dev)
            small_d, big_d = small.to(dev), big.to(dev)
            check(lib.latte_debug_lora_outer(ptr(small_d), ptr(big_d), ptr(buf), ptr(ws), chunks * r * K, M, K, r, chunk, kr, 0, None, DT[dt],
                                             stream_ptr()))
            torch.cuda.synchronize()
            want = small64[:, :r].T @ big64                    # [r, K]
            terms = small64[:, :r].abs().T @ big64.abs()
            out = buf[:r * K].view(K, r).T if kr else buf[:r * K].view(r, K)
            check_elems(f"outer {dt} r{r} kr{kr} M{M} K{K}", out, want, (M + 2) * U32 * terms)   # M additions, lo / L, the join
            assert bool((buf[r * K:] == SENT).all()) and bool((ws[chunks * r * K:] == SENT).all())
            assert bool(torch.isfinite(ws[:chunks * r * K]).all()) and not bool((ws[:chunks * r * K] == SENT).any())


def test_outer_accumulates_and_unscales(lib, dev):
    """Accumulate mode: the reduction adds sum / scale to what the gradient buffer holds (the store launch_split_reduce already has)."""
    g = torch.Generator().manual_seed(7)
    M, K, r, dt = 192, 384, 16, "f16"
    small, small64 = half_randn((M, 2 * r), g, dt)
    small64 = small64[:, :r] + small64[:, r:] / LO[dt]
    big, big64 = half_randn((M, K), g, dt)
    prev = torch.randn(r, K, generator=g)
    out = prev.clone().to(dev)
    scale = torch.tensor([4096.0], device=dev)
    ws = torch.empty(3 * r * K, device=dev)
    small_d, big_d = small.to(dev), big.to(dev)
    check(lib.latte_debug_lora_outer(ptr(small_d), ptr(big_d), ptr(out), ptr(ws), ws.numel(), M, K, r, 64, 0, 1, ptr(scale), DT[dt], stream_ptr()))
    torch.cuda.synchronize()
    want = prev.double() + small64.T @ big64 / 4096.0
    terms = prev.double().abs() + small64.abs().T @ big64.abs() / 4096.0
    check_elems("outer accumulate", out, want, (M + 3) * U32 * terms)   # ... and the add into the buffer


def test_refusals(lib, dev):
    x = torch.zeros(64 * 128, dtype=torch.float16, device=dev)
    o = torch.full((64 * 128,), SENT, device=dev)
    assert lib.latte_debug_lora_down(ptr(x), ptr(x), ptr(x), 64, 128, 12, 1.0, 1, stream_ptr()) != 0          # rank
    assert lib.latte_debug_lora_down(ptr(x), ptr(x), ptr(x), 32, 128, 16, 1.0, 1, stream_ptr()) != 0          # M % 64
    assert lib.latte_debug_lora_down(ptr(x), ptr(x), ptr(x), 64, 64, 16, 1.0, 1, stream_ptr()) != 0           # Kbig % 128
    assert lib.latte_debug_lora_outer(ptr(x), ptr(x), ptr(o), ptr(o), 16 * 128, 64, 128, 16, 32, 0, 0, None, 1, stream_ptr()) != 0   # chunk % 64
    assert lib.latte_debug_lora_outer(ptr(x), ptr(x), ptr(o), ptr(o), 16, 64, 128, 16, 64, 0, 0, None, 1, stream_ptr()) != 0         # workspace
    torch.cuda.synchronize()
    assert bool((o == SENT).all())
    rows = ctypes.c_int()
    n = lib.latte_debug_lora_outer_plan(20480, 768, rows)
    assert rows.value % 64 == 0 and n == -(-20480 // rows.value) and 32 <= n <= 128


# ------------------------------------------------------------------------------------------------ the merged pack
def _arr(ctype, vals):
    return (ctype * len(vals))(*vals)


def _ptr_arr(tensors):
    return _arr(ctypes.c_void_p, [None if t is None else t.data_ptr() for t in tensors])


def _ordered(t):
    """half bit patterns -> integers in value order (sign-magnitude -> two's complement), so that |difference| counts ulps"""
    b = t.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(b < 0, -(b & 0x7FFF), b)


@pytest.mark.parametrize("r", [4, 16, 64])
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_pack_weights_lora(lib, dev, dt, r):
    g = torch.Generator(dev).manual_seed(r)
    D, blocks, s = 128, 2, 2.0 if r != 16 else 0.75
    shapes = [(3 * D, D), (D, D), (4 * D, D), (D, 4 * D)]
    ci = lambda v: _arr(ctypes.c_int, v)
    W, A, B, zB = [], [], [], []
    for i in range(blocks * 4):
        N, K = shapes[i % 4]
        W.append(torch.randn(N, K, generator=g, device=dev) * 0.05)
        targeted = i != 5                                      # block 1's proj is not targeted
        A.append((torch.rand(r, K, generator=g, device=dev) * 2 - 1) * K ** -0.5 if targeted else None)
        B.append(torch.randn(N, r, generator=g, device=dev) * 0.02 if targeted else None)
        zB.append(torch.zeros(N, r, device=dev) if targeted else None)

    def pack(bs, merge=False):
        wn = [torch.full(w.shape, SENT, device=dev, dtype=TD[dt]) for w in W]
        wt = [torch.full((w.shape[1], w.shape[0]), SENT, device=dev, dtype=TD[dt]) for w in W]
        wf = [torch.full(w.shape, SENT, device=dev) for w in W]
        check(lib.latte_debug_pack_weights_lora(_ptr_arr(W), ci([x[0] for x in shapes]), ci([x[1] for x in shapes]),
                                                None if merge else _ptr_arr(wn), None if merge else _ptr_arr(wt),
                                                _ptr_arr(wf) if merge else None, _ptr_arr(A), _ptr_arr(bs), blocks, r, s, DT[dt], stream_ptr()))
        torch.cuda.synchronize()
        return wf if merge else (wn, wt)

    wn, wt = pack(B)
    wf = pack(B, merge=True)
    zn, zt = pack(zB)
    pn = [torch.empty_like(x) for x in wn]
    pt = [torch.empty_like(x) for x in wt]
    check(lib.latte_debug_pack_weights(_ptr_arr(W), ci([x[0] for x in shapes]), ci([x[1] for x in shapes]), _ptr_arr(pn), _ptr_arr(pt), blocks,
                                       DT[dt], stream_ptr()))
    torch.cuda.synchronize()
    i16 = lambda t: t.contiguous().view(torch.int16)
    for i, w in enumerate(W):
        assert torch.equal(i16(zn[i]), i16(pn[i])) and torch.equal(i16(zt[i]), i16(pt[i])), i          # B = 0: the plain pack's bits
        assert torch.equal(i16(wt[i]), i16(wn[i].t().contiguous())), i                                  # one value, two layouts
        if A[i] is None:
            assert torch.equal(i16(wn[i]), i16(pn[i])) and bool((wf[i] == SENT).all()), i               # untargeted: W itself, not merged
            continue
        ref32 = w + s * (B[i] @ A[i])                                                                   # torch fp32
        assert int((_ordered(wn[i]) - _ordered(ref32.to(TD[dt]))).abs().max()) <= 1, i
        assert torch.equal(i16(wf[i].to(TD[dt])), i16(wn[i])), i                                        # merge, then the plain rounding
        ref64 = w.double() + s * (B[i].double() @ A[i].double())
        terms = w.double().abs() + s * (B[i].double().abs() @ A[i].double().abs())
        assert not bool(((wf[i].double() - ref64).abs() > (r + 2) * U32 * terms).any()), i
        assert not torch.equal(i16(wn[i]), i16(pn[i])), i                                               # the adapters did reach the operand
