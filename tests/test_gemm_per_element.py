"""The MFMA GEMMs (csrc/gemm.hip, csrc/gemm_pw.hip) with every epilogue, and ln_modulate_kernel (csrc/pointwise.hip), per element against
fp64 on the same half-rounded operands -- through latte_debug_gemm (variants 1-9, 12, 13, 18, 19, 10, 11 and 0 = the launcher's choice;
epilogues 0 bias -> half, 1 bias + GELU -> half, 2 gated fp32 read-modify-write, 3 bias -> fp32, 5 bias + half residual -> half),
latte_debug_gemm_gelu (13: u and GELU(u), 14: (A W^T + bias) gelu'(u)) and latte_debug_ln_modulate.  u = 2^-8 (bf16) / 2^-11 (f16) is the
unit roundoff of the half type, e = 2^-24 that of fp32, 2^-25 the rounding error among the f16 subnormals.

GEMM BOUND.  want = A W^T + bias in fp64, S = sum_k |a_k| |w_k|.
  accumulator + bias     (K + 3) e (S + |bias|): the any-order bound of a sum of K exact products (a product of two halves is exact in
                         fp32) and the bias (epilogue_store: `a[0] + b4.x`).  It assumes that each addition inside an MFMA is no worse
                         than one fp32 rounding.
  half outputs (0, 1, 5, 13, 14)   + u |want| (pack2), f16: + 2^-25.
  epi 3                  nothing more: the bias add is the last operation.
  epi 1, 13, 14          gelu_tanh(x) = x gelu_sig(x), gelu_sig = rcp(1 + exp2(p x)), p = fma(x x, a1, a0) (device_util.h; gemm_pw.hip
                         repeats the expression), a0 = -2 log2(e) sqrt(2 / pi), a1 = 0.044715 a0.  The exp2 argument t = p x carries
                         dt <= e (2 |a1 x^3| + |a0 x| + 2 |t|): the constants a1 and a0 as floats, the square, the fma, the product.
                         exp2: one ulp = 2 e; 1 + E: e; rcp: RCP (below); the product with x: e.  Relative to gelu(x):
                         (1 - sig) (ln2 dt + 2 e) + 2 e + RCP, 1 - sig = E / (1 + E).  The argument's own error (the accumulator's) goes
                         through |d gelu / dx| <= 1.13.
                         RCP: no ISA document is installed with the toolchain, so the second route of DESIGN.md section 4.6: the worst
                         relative deviation of torch's CPU fp32 reciprocal from fp64 over a fixed grid of [1, 2), times four (4 x 2^-24).
  epi 13                 out = half(u), u = A W^T + bias, as epi 0; aux = half(gelu(float(out))): the GELU of the ROUNDED u, so the
                         reference is the fp64 GELU of the kernel's own `out` and the chain has no argument error.
  epi 14                 out = half(v dgelu(x)), v = A W^T + bias, x = aux (read, exact); dgelu = sg + x sg (1 - sg) 2 du,
                         du = 0.7978845608 (1 + 0.134145 x x).  d_sg = sg ((1 - sg) (ln2 dt + 2 e) + e + RCP); the second term:
                         |x| 2 du (d_sg (1 - sg) + sg (e + d_sg)) for its factors sg and 1 - sg, 9 e relative for du's four operations
                         and two constants and the three products; the sum e.  Then |dv| |dgelu| + |v| d_dgelu + e |v dgelu|.
  epi 2                  out = out0 + gate v: |gate| times the accumulator term, e |gate want| for the product and e (|out0| +
                         |gate want|) for the read-modify-write add.  `r.x += g4.x * v0` is a contractible pair and the gfx950 code object
                         holds v_pk_fma_f32 there (read in the compiler's listing, as for gated_split_reduce in section 4.6): fused, the
                         product's rounding disappears.  The bound keeps it and so covers both forms; the stand-in takes the fused one.
  epi 5                  v + res in fp32 (the half residual is decoded exactly; the add rounds once: e |want|), then the half rounding.

EDGES, each exact.  Rows M..Mpad of A hold NaN (even cases) or +Inf (odd cases): every valid row keeps the bits it has with finite
padding.  `out` (and `aux`) is NaN before every launch that overwrites it and lies between guard rows in front and behind that must come
back bit for bit.  Epi 2 at rows_per_sample 64, 256, 4096 and 100, 72, 1 (a sample boundary inside a 16-row fragment; variant 18 falls back
to its producer form, variants 7-11 leave the whole-tiles-in-one-sample path) with gate_stride 2 N + 8 > 2 N, the gate columns >= N NaN.
Epi 5 with `res` aliasing `out` gives the bits of the launch that keeps them apart.

LN-MODULATE BOUND (pointwise.hip: ln_modulate_kernel).  A wave holds a row, a lane NQ = ceil(D / 256) float4 chunks.
  x + temp_embed         one fp32 add, written back: equal to torch's fp32 add bit for bit; everything below starts from it.
  mean                   per lane NQ terms of three adds each `(x + y) + (z + w)` plus the running sum, the six steps of wave_sum, the
                         constant 1 / D and its product: n = 4 NQ + 8 roundings on the path of an element: dmean <= n e sum |x| / D.
  variance               a = x - mean (e |a|, twice in a a), the square, then the same chain: (n + 3) e var; a wrong mean adds dmean^2
                         exactly (the centred sum of x is zero) -- the kernel is two-pass, the offset does not enter at first order.
  rstd                   1.0f / sqrtf(var + 1e-6f): the sum, the root and the division, e each: drstd <= 1/2 rstd^3 dvar + 3 e rstd.
  out                    (x - mean) rstd (1 + scale) + shift: [(dmean + e |xc|) rstd + |xc| drstd] |1 + scale| for the operands,
                         3 e |xc rstd (1 + scale)| for 1 + scale and the two products, e |out| for the sum; then u |want|, f16 + 2^-25.
Rows have their own sigma in [1/4, 4] and a mean of 0, 4 or 32 sigma.  RECORDED, not asserted: the worst deviation of y from the fp64
LayerNorm per offset, in half ulps of the element (u |want|) and of the two terms that form it (u (|xc rstd (1 + scale)| + |shift|),
which an output near zero does not inflate) -- what the fp32 mean costs at |mean| / sigma = 32.

The CPU half (not marked gpu) runs torch stand-ins that round where the kernels round through the same bounds on the same cases, and
shows that named mistakes leave them (the GEMM stand-in on the shapes of up to 5.4 GFLOP, whose fp64 products take seconds on a CPU; it
does not depend on the tile variant); two of the GEMM mistakes stay under the norm-wise tolerance of tests/test_gpu_kernels.py.

Worst err / bound per variant and epilogue on the MI355X: DESIGN.md section 4.11."""
import math

import pytest
import torch

gpu = pytest.mark.gpu
TD = {0: torch.bfloat16, 1: torch.float16}
DTN = {0: "bf16", 1: "f16"}
U_HALF = {0: 2.0 ** -8, 1: 2.0 ** -11}
ETA = {0: 0.0, 1: 2.0 ** -25}
U32 = 2.0 ** -24
LN2 = math.log(2.0)
A0 = -2.0 * 1.4426950408889634 * math.sqrt(2.0 / math.pi)
A1 = 0.044715 * A0
TINY = 2.0 ** -120            # exp2 / rcp flush what lies below 2^-126
GUARD = 3
SENT = -7.25
OUT_TOL = {0: 6e-3, 1: 1e-3}  # tests/test_gpu_kernels.py


def _rcp_rel():
    x = 1.0 + torch.arange(1 << 16, dtype=torch.float64) / (1 << 16) + 2.0 ** -20 / 3
    x32 = x.float()
    return 4.0 * float(((1.0 / x32).double() * x32.double() - 1.0).abs().max())


RCP = _rcp_rel()

SHAPES = [(256, 256, 128), (512, 768, 1152), (300, 512, 256), (1024, 1152, 4608), (700, 384, 64), (8292, 2304, 192), (8292, 2432, 192),
          (300, 288, 64), (130, 144, 128), (4096, 1152, 1152),                             # test_gemm_epilogues
          (8192, 1152, 4608), (33000, 1152, 1152), (2304, 384, 256)]                       # test_gemm_producer_wave_kernel
VARIANTS = [1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 13, 18, 19, 10, 11, 0]
TILE_N = {0: 64, 1: 128, 2: 128, 3: 256, 4: 128, 5: 192, 6: 256, 7: 32, 8: 48, 9: 64, 10: 192, 11: 192, 12: 144, 13: 144, 18: 144, 19: 144}
RPS = [64, 256, 4096, 100, 72, 1]


def runs(variant, shape):
    """the skip rules of test_gemm_epilogues"""
    M, N, K = shape
    if N % TILE_N[variant]:
        return False
    if 7 <= variant <= 11 and K < 128 and (variant >= 10 or N % (4 * TILE_N[variant])):
        return False
    return True


GEMM_CASES = [(s, dt, v) for s in SHAPES for dt in (0, 1) for v in VARIANTS if runs(v, s)]
GELU_CASES = [(s, dt) for s in SHAPES for dt in (0, 1) if s[1] % 192 == 0 and s[2] >= 128]


def _gid(c):
    return "-".join(["x".join(str(i) for i in c[0]), DTN[c[1]]] + [f"v{v}" for v in c[2:]])


def rps_list(M):
    return [r for r in RPS if r != 1 or M <= 1024]


# ------------------------------------------------------------------------------------------------ operands, fp64 references, bounds
class Operands:
    """One (shape, dtype): A [Mpad, K] (rows >= M: N(0, 1); a_pad(kind) gives the NaN / +Inf forms), W, bias, res, out0, the gates, and the
    fp64 product with S.  Built once per (shape, dtype, device) and shared by every variant (the tests leave it unchanged)."""
    _last = None

    @classmethod
    def get(cls, shape, dt, dev):
        key = (shape, dt, dev.type)
        if cls._last is None or cls._last.key != key:
            cls._last = None
            cls._last = cls(shape, dt, dev)
            cls._last.key = key
        return cls._last

    def __init__(self, shape, dt, dev):
        M, N, K = shape
        self.M, self.N, self.K, self.dt, self.dev = M, N, K, dt, dev
        g = torch.Generator(dev).manual_seed(M + N + K + dt)
        self.Mp = Mp = (M + 255) // 256 * 256
        self.A = torch.randn(Mp, K, generator=g, device=dev).to(TD[dt])
        self.W = (torch.randn(N, K, generator=g, device=dev) / K ** 0.5).to(TD[dt])
        self.bias = torch.randn(N, generator=g, device=dev)
        self.res = torch.randn(M, N, generator=g, device=dev).to(TD[dt])
        self.out0 = torch.randn(M, N, generator=g, device=dev)
        self.gates = {}
        for rps in rps_list(M):
            stride = 2 * N if rps == 64 else 2 * N + 8
            gate = torch.full(((M + rps - 1) // rps, stride), float("nan"), device=dev)
            gate[:, :N] = torch.randn(gate.shape[0], N, generator=g, device=dev)
            self.gates[rps] = gate
        Ad, Wd = self.A[:M].double(), self.W.double()
        self.prod = Ad @ Wd.t()
        self.acc_b = (K + 3) * U32 * ((Ad.abs() @ Wd.abs().t()) + self.bias.double().abs())
        self.want = self.prod + self.bias.double()
        self._pad = {}

    def a_pad(self, kind):
        """A with its rows >= M filled with NaN or +Inf"""
        if self.Mp == self.M:
            return self.A
        if kind not in self._pad:
            a = self.A.clone()
            a[self.M:] = kind
            self._pad = {kind: a}
        return self._pad[kind]

    def gate_rows(self, rps):
        return self.gates[rps][torch.arange(self.M, device=self.dev) // rps, :self.N].double()


def gelu_ref(x):
    """fp64 GELU(tanh) of x and the relative bound of the kernel's chain on an exact argument -> (want, rel)"""
    p = A0 + A1 * x * x
    t = p * x
    sig = torch.sigmoid(-t * LN2)
    dt_ = U32 * (2 * (A1 * x ** 3).abs() + (A0 * x).abs() + 2 * t.abs())
    return x * sig, (1 - sig) * (LN2 * dt_ + 2 * U32) + 2 * U32 + RCP


def dgelu_ref(x):
    """fp64 gelu'(x) and the absolute bound of the kernel's dgelu chain on an exact argument"""
    p = A0 + A1 * x * x
    t = p * x
    sg = torch.sigmoid(-t * LN2)
    du = math.sqrt(2.0 / math.pi) * (1 + 3 * 0.044715 * x * x)
    term2 = x * sg * (1 - sg) * 2 * du
    dt_ = U32 * (2 * (A1 * x ** 3).abs() + (A0 * x).abs() + 2 * t.abs())
    d_sg = sg * ((1 - sg) * (LN2 * dt_ + 2 * U32) + U32 + RCP)
    want = sg + term2
    return want, d_sg + x.abs() * 2 * du * (d_sg * (1 - sg) + sg * (U32 + d_sg)) + 9 * U32 * term2.abs() + U32 * want.abs()


def half_bound(dt, want, inner):
    return inner * (1 + U_HALF[dt]) + U_HALF[dt] * want.abs() + ETA[dt] + TINY


def expected(op, epi, rps=None, u_out=None, aux=None):
    """-> (want, bound), fp64 [M, N], of out for an epilogue (module docstring); epi "13aux": of aux given the kernel's own out"""
    dt = op.dt
    if epi == 0 or epi == 13:
        return op.want, half_bound(dt, op.want, op.acc_b)
    if epi == 3:
        return op.want, op.acc_b
    if epi == 1:
        want, rel = gelu_ref(op.want)
        return want, half_bound(dt, want, 1.13 * op.acc_b + rel * want.abs())
    if epi == 2:
        gate = op.gate_rows(rps)
        gw = gate * op.want
        return op.out0.double() + gw, gate.abs() * op.acc_b + U32 * gw.abs() + U32 * (op.out0.double().abs() + gw.abs())
    if epi == 5:
        want = op.want + op.res.double()
        return want, half_bound(dt, want, op.acc_b + U32 * want.abs())
    if epi == "13aux":
        want, rel = gelu_ref(u_out.double())
        return want, half_bound(dt, want, rel * want.abs())
    if epi == 14:
        d, dd = dgelu_ref(aux.double())
        want = op.want * d
        return want, half_bound(dt, want, op.acc_b * d.abs() + op.want.abs() * dd + U32 * want.abs())
    raise ValueError(epi)


def worst(tag, got, want, bound, raise_=True):
    err = (got.double() - want).abs()
    bad = ~(err <= bound)
    ratio = float(torch.nan_to_num(err / bound, nan=float("inf")).max())
    if raise_ and bool(bad.any()):
        i = tuple(int(t) for t in torch.nonzero(bad)[0])
        raise AssertionError(f"{tag}: {int(bad.sum())} of {err.numel()} elements out of bound; first (row, column) {i}: got {float(got[i]):.6e} "
                             f"want {float(want[i]):.6e} err {float(err[i]):.3e} > {float(bound[i]):.3e}; worst err / bound {ratio:.3f}")
    return ratio


# ------------------------------------------------------------------------------------------------ the kernels restated in fp32
GEMM_MISTAKES = ("subtile_skips_k_tile", "fragment_zero", "lane_store_skipped", "gate_of_first_row", "bias_4_off", "res_element_0")


def _fma(a, b, c):
    """fp32 fused multiply-add: the product of two floats is exact in fp64, the sum is rounded there and again to fp32"""
    return (a.double() * b.double() + c.double()).float()


def _gelu32(x):
    p = _fma(x * x, torch.tensor(-0.10294324), torch.tensor(-2.3022082))
    return x * (1.0 / (1.0 + torch.exp2(p * x)))


def _dgelu32(x):
    p = _fma(x * x, torch.tensor(-0.10294324), torch.tensor(-2.3022082))
    sg = 1.0 / (1.0 + torch.exp2(p * x))
    du = torch.tensor(0.7978845608) * (1.0 + torch.tensor(0.134145) * x * x)
    return sg + x * sg * (1.0 - sg) * 2.0 * du


def gemm_standin(op, epi, rps=None, aux=None, mistake=None, init=None):
    """fp32 torch on the half operands + the epilogue's own operations -> out [M, N] (half or fp32), for epi 13 (out, aux).  A mistake
    touches one place: rows 64.., columns 64.. (the second wave sub-tile), the last valid row, or the epilogue's side operand."""
    M, N, K, dt = op.M, op.N, op.K, op.dt
    A, W = op.A[:M].float(), op.W.float()
    acc = A @ W.t()
    r0, c0 = min(64, M - 16) // 16 * 16, min(64, N - 16) // 16 * 16
    if mistake == "subtile_skips_k_tile":
        acc[r0:r0 + 64, c0:c0 + 64] -= A[r0:r0 + 64, K - 64:] @ W[c0:c0 + 64, K - 64:].t()
    if mistake == "fragment_zero":
        acc[r0:r0 + 16, c0:c0 + 16] = 0.0
    bias = op.bias.roll(-4) if mistake == "bias_4_off" else op.bias
    v = acc + bias
    if epi in (0, 13):
        out = v.to(TD[dt])
    elif epi == 1:
        out = _gelu32(v).to(TD[dt])
    elif epi == 3:
        out = v
    elif epi == 2:
        rows = torch.arange(M) // rps
        if mistake == "gate_of_first_row":
            rows = (torch.arange(M) // 256 * 256) // rps
        out = _fma(op.gates[rps][rows, :N], v, op.out0)          # the code object holds the fused form
    elif epi == 5:
        res = op.res.float()
        if mistake == "res_element_0" and dt == 1:
            res = res.view(M, N // 4, 4)[:, :, :1].expand(-1, -1, 4).reshape(M, N)
        out = (v + res).to(TD[dt])
    elif epi == 14:
        out = (v * _dgelu32(aux.float())).to(TD[dt])
    if mistake == "lane_store_skipped":
        out = out.clone()
        out[M - 1, c0:c0 + 4] = init[M - 1, c0:c0 + 4] if init is not None else float("nan")
    if epi == 13:
        return out, _gelu32(out.float()).to(TD[dt])
    return out


CPU_SHAPES = [s for s in SHAPES if s[0] * s[1] * s[2] <= 1024 * 1152 * 4608]      # fp64 products of up to 5.4 GFLOP: seconds on a CPU


@pytest.mark.parametrize("shape", CPU_SHAPES, ids=lambda s: "x".join(str(i) for i in s))
@pytest.mark.parametrize("dt", [0, 1], ids=["bf16", "f16"])
def test_gemm_standin_within_bounds(shape, dt):
    """the restated epilogues pass what the GPU results have to pass (the stand-in does not depend on the tile variant)"""
    op = Operands.get(shape, dt, torch.device("cpu"))
    res = {}
    for epi in (0, 1, 3, 5, 14):
        aux = op.res if epi == 14 else None          # any half tensor serves as the pre-activation u of epi 14
        want, bound = expected(op, epi, aux=aux)
        res[epi] = worst(f"epi {epi}", gemm_standin(op, epi, aux=aux), want, bound)
    u_out, aux = gemm_standin(op, 13)
    res[13] = worst("epi 13 aux", aux, *expected(op, "13aux", u_out=u_out))
    for rps in rps_list(op.M):
        want, bound = expected(op, 2, rps=rps)
        res[f"2/{rps}"] = worst(f"epi 2 rps {rps}", gemm_standin(op, 2, rps=rps), want, bound)
    assert max(res.values()) < 1.0
    print(f"gemm stand-in {_gid((shape, dt))}: " + " ".join(f"{k}: {v:.3f}" for k, v in res.items()))


@pytest.mark.parametrize("mistake", GEMM_MISTAKES)
def test_gemm_named_mistakes_leave_the_bounds(mistake):
    """One mistake at a time over four small shapes, both dtypes, the epilogues it can show in; failing / tried as run on the CPU:
    subtile_skips_k_tile 32 / 32, fragment_zero 32 / 32, lane_store_skipped 32 / 32, gate_of_first_row 24 / 32 (every rows_per_sample but 256
    in shapes of more than one sample), bias_4_off 32 / 32, res_element_0 4 / 4 (f16 only: the bf16 decode has no such form)."""
    tried, failed = 0, 0
    for shape in [(256, 256, 128), (300, 512, 256), (700, 384, 64), (130, 144, 128)]:
        for dt in (0, 1):
            op = Operands.get(shape, dt, torch.device("cpu"))
            if mistake == "gate_of_first_row":
                todo = [(2, r) for r in (64, 256, 100, 72)]
            elif mistake == "res_element_0":
                todo = [(5, None)] if dt == 1 else []
            else:
                todo = [(0, None), (1, None), (2, 100), (3, None)]
            for epi, rps in todo:
                want, bound = expected(op, epi, rps=rps)
                got = gemm_standin(op, epi, rps=rps, mistake=mistake, init=op.out0 if epi == 2 else None)
                tried += 1
                failed += worst("", got, want, bound, raise_=False) > 1.0
    print(f"{mistake}: {failed} of {tried} fail")
    assert failed > 0


@pytest.mark.parametrize("shape,mistake", [((1024, 1152, 4608), "subtile_skips_k_tile"), ((8292, 2304, 192), "fragment_zero")])
def test_localised_gemm_mistakes_pass_the_norm_wise_test(shape, mistake):
    """Why this file exists: on test_gemm_epilogues' own operands (its seed, N(0, 1) A, W / sqrt(K)) in bf16, one wave sub-tile that skips a
    K tile and one accumulator fragment left at zero stay under its whole-tensor tolerance of 6e-3, and leave the per-element bound."""
    M, N, K = shape
    dt = 0
    g = torch.Generator("cpu").manual_seed(M + N + K)
    Mp = (M + 255) // 256 * 256
    op = Operands.__new__(Operands)
    op.M, op.N, op.K, op.dt, op.Mp = M, N, K, dt, Mp
    op.A = torch.randn(Mp, K, generator=g).to(TD[dt])
    op.W = (torch.randn(N, K, generator=g) / K ** 0.5).to(TD[dt])
    op.bias = torch.randn(N, generator=g)
    ref = op.A.float()[:M] @ op.W.float().t() + op.bias
    clean = gemm_standin(op, 0)
    bad = gemm_standin(op, 0, mistake=mistake)
    rel = {k: float((t.float() - ref).norm() / ref.norm()) for k, t in (("clean", clean), ("bad", bad))}
    print(f"{shape} {mistake}: clean {rel['clean']:.2e}, with the mistake {rel['bad']:.2e}, tolerance {OUT_TOL[dt]:.0e}")
    assert rel["bad"] < OUT_TOL[dt]
    Ad, Wd = op.A[:M].double(), op.W.double()
    op.want = Ad @ Wd.t() + op.bias.double()
    op.acc_b = (K + 3) * U32 * ((Ad.abs() @ Wd.abs().t()) + op.bias.double().abs())
    want, bound = expected(op, 0)
    assert worst("", clean, want, bound, raise_=False) < 1.0
    assert worst("", bad, want, bound, raise_=False) > 1.0


# ------------------------------------------------------------------------------------------------ LN-modulate: inputs, reference, stand-in
LN_B = 2
# (D, use_te, dt, F, T, M, offset): rows_per_sample = F T; M = 128 whole samples, and M = 126 with rows_per_sample 63 (M % 4 != 0, a
# 4-row block that holds two samples)
LN_CASES = [(D, te, dt, 4, 16, 128, (0, 4, 32)[(i + te + dt) % 3]) for i, D in enumerate([128, 384, 768, 1024, 1152]) for te in (0, 1) for dt in (0, 1)]
LN_CASES += [(1152, 1, 0, 7, 9, 126, 32), (384, 0, 1, 7, 9, 126, 4), (128, 1, 1, 7, 9, 126, 0)]
LN_CASES += [(1152, 0, 1, 4, 16, 128, off) for off in (0, 4, 32)] + [(768, 1, 0, 4, 16, 128, off) for off in (0, 4, 32)]      # the offset table
LN_CASES = list(dict.fromkeys(LN_CASES))


def _lid(c):
    D, te, dt, F, T, M, off = c
    return f"D{D}-te{te}-{DTN[dt]}-F{F}-T{T}-M{M}-off{off}"


def ln_inputs(case, dev):
    """-> x [M + 1, D] fp32 (row M: what lies behind the last row, finite), mod [B, 6 D + 8], te [F, D]"""
    D, use_te, dt, F, T, M, off = case
    g = torch.Generator(dev).manual_seed(D + 7 * off + M)
    sigma = 2.0 ** (torch.rand(M + 1, 1, generator=g, device=dev) * 4 - 2)
    sign = torch.where(torch.rand(M + 1, 1, generator=g, device=dev) < 0.5, -1.0, 1.0)
    x = torch.randn(M + 1, D, generator=g, device=dev) * sigma + sign * off * sigma
    mod = torch.randn(LN_B, 6 * D + 8, generator=g, device=dev)
    te = torch.randn(F, D, generator=g, device=dev)
    return x, mod, te


def ln_expected(case, xr, mod):
    """xr [M, D]: the fp32 rows the LayerNorm starts from (after the temp_embed add) -> (want, bound, |xc rstd (1 + scale)| + |shift|) fp64"""
    D, use_te, dt, F, T, M, off = case
    xd = xr.double()
    smp = torch.arange(M, device=xr.device) // (F * T)
    shift, scale = mod[smp, :D].double(), mod[smp, D:2 * D].double()
    n = 4 * ((D // 4 + 63) // 64) + 8
    mean = xd.mean(-1, keepdim=True)
    xc = xd - mean
    var = (xc * xc).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + float(torch.tensor(1e-6, dtype=torch.float32)))
    dmean = n * U32 * xd.abs().mean(-1, keepdim=True)
    dvar = (n + 3) * U32 * var + dmean * dmean
    drstd = 0.5 * rstd ** 3 * dvar + 3 * U32 * rstd
    core = xc * rstd * (1 + scale)
    want = core + shift
    inner = ((dmean + U32 * xc.abs()) * rstd + xc.abs() * drstd) * (1 + scale).abs() + 3 * U32 * core.abs() + U32 * want.abs()
    return want, half_bound(dt, want, inner), core.abs() + shift.abs()


LN_MISTAKES = ("sample_per_block", "last_group_summed_in_full")


def ln_standin(case, x, mod, te, mistake=None):
    """ln_modulate_kernel in torch fp32, a lane's chunks and the wave reduction in the kernel's order -> (x after the add [M, D], y half)"""
    D, use_te, dt, F, T, M, off = case
    dev = x.device
    rows = torch.arange(M, device=dev)
    xr = x[:M] + te[(rows // T) % F] if use_te else x[:M].clone()
    NT = D // 4
    NQ = (NT + 63) // 64
    v = torch.zeros(M, NQ * 64, 4, device=dev)
    v[:, :NT] = xr.view(M, NT, 4)
    summed = v.clone()
    if mistake == "last_group_summed_in_full" and NT % 64:      # the lanes without a chunk read on: the next row's first elements
        nxt = torch.cat([xr[1:], x[M:M + 1]]).view(M, NT, 4)
        summed[:, NT:] = nxt[:, :NQ * 64 - NT]
    inv_d = torch.tensor(1.0, dtype=torch.float32) / D

    def lanes(t):           # [M, NQ * 64, 4] -> per-lane chain -> wave_sum (xor 32, 16, ..., 1) -> [M, 1]
        t = t.view(M, NQ, 64, 4)
        s = torch.zeros(M, 64, device=dev)
        for c in range(NQ):
            s = s + ((t[:, c, :, 0] + t[:, c, :, 1]) + (t[:, c, :, 2] + t[:, c, :, 3]))
        lane = torch.arange(64, device=dev)
        for o in (32, 16, 8, 4, 2, 1):
            s = s + s[:, lane ^ o]
        return s[:, :1]

    mean = lanes(summed) * inv_d
    a = summed - mean.unsqueeze(-1)
    if mistake != "last_group_summed_in_full":
        a[:, NT:] = 0.0
    rstd = 1.0 / torch.sqrt(lanes(a * a) * inv_d + torch.tensor(1e-6))
    smp = rows // (F * T)
    if mistake == "sample_per_block":
        smp = (rows // 4 * 4) // (F * T)
    shift, scale = mod[smp, :D], mod[smp, D:2 * D]
    y = (xr - mean) * rstd * (1.0 + scale) + shift
    return xr, y.to(TD[dt])


def _half_ulps(got, want, mag, dt):
    """the deviation from the fp64 LayerNorm in half ulps (u |want|) of the element itself -- outputs near zero, where the modulated value
    cancels the shift, dominate it -- and in half ulps of the two terms that form it, u (|xc rstd (1 + scale)| + |shift|)"""
    dev = (got.double() - want).abs()
    return (f"{float((dev / (U_HALF[dt] * want.abs()).clamp(min=2.0 ** -24)).max()):.2f} half ulps of the element, "
            f"{float((dev / (U_HALF[dt] * mag).clamp(min=2.0 ** -24)).max()):.3f} half ulps of its terms from the fp64 LayerNorm")


@pytest.mark.parametrize("case", LN_CASES, ids=_lid)
def test_ln_standin_within_bound(case):
    x, mod, te = ln_inputs(case, torch.device("cpu"))
    xr, y = ln_standin(case, x, mod, te)
    want, bound, mag = ln_expected(case, xr, mod)
    ratio = worst(_lid(case), y, want, bound)
    assert ratio < 1.0
    print(f"ln_modulate stand-in {_lid(case)}: worst err / bound {ratio:.3f}, {_half_ulps(y, want, mag, case[2])}")


@pytest.mark.parametrize("mistake", LN_MISTAKES)
def test_ln_named_mistakes_leave_the_bound(mistake):
    """sample_per_block shows where a 4-row block holds two samples (rows_per_sample 63: 3 of 3 cases); last_group_summed_in_full where the
    last chunk group is half populated (D = 128, 384, 1152: 17 of 17 cases, none at D = 768, 1024)."""
    tried, failed = 0, 0
    for case in LN_CASES:
        D, use_te, dt, F, T, M, off = case
        if (mistake == "sample_per_block" and (F * T) % 4 == 0) or (mistake == "last_group_summed_in_full" and (D // 4) % 64 == 0):
            continue
        x, mod, te = ln_inputs(case, torch.device("cpu"))
        xr, y = ln_standin(case, x, mod, te, mistake)
        tried += 1
        failed += worst("", y, *ln_expected(case, xr, mod)[:2], raise_=False) > 1.0
    print(f"{mistake}: {failed} of {tried} fail")
    assert failed > 0


# ------------------------------------------------------------------------------------------------ GPU
def _guarded(M, N, dtype, dev, init=None):
    """-> (buffer, view [M, N]): GUARD sentinel rows in front and behind, the view NaN or a copy of init"""
    buf = torch.full((M + 2 * GUARD, N), SENT, dtype=dtype, device=dev)
    view = buf[GUARD:GUARD + M]
    if init is None:
        view.fill_(float("nan"))
    else:
        view.copy_(init)
    return buf, view


def _guards_intact(tag, buf, M):
    sent = torch.full_like(buf[:GUARD], SENT)
    assert torch.equal(buf[:GUARD], sent), f"{tag}: wrote in front of out"
    assert torch.equal(buf[GUARD + M:], sent), f"{tag}: wrote behind out"


def _same_bits(a, b):
    return torch.equal(a.view(torch.int16 if a.element_size() == 2 else torch.int32), b.view(torch.int16 if b.element_size() == 2 else torch.int32))


def _gemm(lib, op, A, out, side, rps, gate_stride, epi, variant):
    from latte_amd._lib import check, ptr, stream_ptr
    check(lib.latte_debug_gemm(ptr(A), ptr(op.W), ptr(op.bias), ptr(out), ptr(side), op.M, op.N, op.K, gate_stride, rps, epi, op.dt, variant,
                               stream_ptr()))
    torch.cuda.synchronize()


@gpu
@pytest.mark.parametrize("case", GEMM_CASES, ids=_gid)
def test_gemm_per_element(lib, case):
    shape, dt, variant = case
    dev = torch.device("cuda")
    op = Operands.get(shape, dt, dev)
    M, N = op.M, op.N
    pad = float("nan") if (M + N + variant) % 2 == 0 else float("inf")
    A_pad = op.a_pad(pad)
    res = {}
    for epi in (0, 1, 3) + ((5,) if variant in (1, 2, 3) else ()):
        tag = f"{_gid(case)} epi {epi}"
        outs = []
        for A in (A_pad, op.A):
            buf, out = _guarded(M, N, torch.float32 if epi == 3 else TD[dt], dev)
            _gemm(lib, op, A, out, op.res if epi == 5 else None, M, 0, epi, variant)
            _guards_intact(tag, buf, M)
            outs.append(out)
        assert _same_bits(outs[0], outs[1]), f"{tag}: the rows behind M of A reach valid rows"
        res[epi] = worst(tag, outs[0], *expected(op, epi))
        if epi == 5:                                   # res aliasing out (the VAE's call): same bits
            buf, out = _guarded(M, N, TD[dt], dev, init=op.res)
            _gemm(lib, op, A_pad, out, out, M, 0, 5, variant)
            _guards_intact(tag + " in place", buf, M)
            assert _same_bits(out, outs[0]), f"{tag}: in place differs"
    for rps in rps_list(M):
        tag = f"{_gid(case)} epi 2 rows_per_sample {rps}"
        gate = op.gates[rps]
        buf, out = _guarded(M, N, torch.float32, dev, init=op.out0)
        _gemm(lib, op, A_pad, out, gate, rps, gate.shape[1], 2, variant)
        _guards_intact(tag, buf, M)
        res[f"2/{rps}"] = worst(tag, out, *expected(op, 2, rps=rps))
        if rps == 64:
            buf, out_f = _guarded(M, N, torch.float32, dev, init=op.out0)
            _gemm(lib, op, op.A, out_f, gate, rps, gate.shape[1], 2, variant)
            assert _same_bits(out, out_f), f"{tag}: the rows behind M of A reach valid rows"
    print(f"gemm {_gid(case)}: err / bound " + " ".join(f"{k}: {v:.3f}" for k, v in res.items()))


@gpu
@pytest.mark.parametrize("case", GELU_CASES, ids=_gid)
def test_gemm_gelu_training_epilogues_per_element(lib, case):
    from latte_amd._lib import check, ptr, stream_ptr
    shape, dt = case
    dev = torch.device("cuda")
    op = Operands.get(shape, dt, dev)
    M, N, K = shape
    A_pad = op.a_pad(float("nan") if (M + N) % 2 == 0 else float("inf"))
    got = []
    for A in (A_pad, op.A):
        ubuf, u = _guarded(M, N, TD[dt], dev)
        hbuf, h = _guarded(M, N, TD[dt], dev)
        check(lib.latte_debug_gemm_gelu(ptr(A), ptr(op.W), ptr(op.bias), ptr(u), ptr(h), M, N, K, 13, dt, stream_ptr()))
        torch.cuda.synchronize()
        _guards_intact("epi 13 out", ubuf, M)
        _guards_intact("epi 13 aux", hbuf, M)
        got.append((u, h))
    assert _same_bits(got[0][0], got[1][0]) and _same_bits(got[0][1], got[1][1]), "the rows behind M of A reach valid rows"
    u, h = got[0]
    r13 = worst(f"{_gid(case)} epi 13 out", u, *expected(op, 13))
    r13a = worst(f"{_gid(case)} epi 13 aux", h, *expected(op, "13aux", u_out=u))
    # epi 14 reads the pre-activation from aux, rows clamped at M - 1: Mpad rows are not needed
    dbuf, du = _guarded(M, N, TD[dt], dev)
    u_in = u.clone()
    check(lib.latte_debug_gemm_gelu(ptr(A_pad), ptr(op.W), ptr(op.bias), ptr(du), ptr(u_in), M, N, K, 14, dt, stream_ptr()))
    torch.cuda.synchronize()
    _guards_intact("epi 14 out", dbuf, M)
    assert _same_bits(u_in, u), "epi 14 wrote its aux"
    r14 = worst(f"{_gid(case)} epi 14", du, *expected(op, 14, aux=u))
    print(f"gemm_gelu {_gid(case)}: err / bound 13: {r13:.3f} 13aux: {r13a:.3f} 14: {r14:.3f}")


@gpu
@pytest.mark.parametrize("case", LN_CASES, ids=_lid)
def test_ln_modulate_per_element(lib, case):
    from latte_amd._lib import check, ptr, stream_ptr
    D, use_te, dt, F, T, M, off = case
    dev = torch.device("cuda")
    x, mod, te = ln_inputs(case, dev)
    xbuf, xin = _guarded(M, D, torch.float32, dev, init=x[:M])
    ybuf, y = _guarded(M, D, TD[dt], dev)
    check(lib.latte_debug_ln_modulate(ptr(xin), ptr(y), ptr(mod), ptr(mod[:, D:]), mod.shape[1], M, D, F * T, ptr(te) if use_te else None, T, F,
                                      dt, stream_ptr()))
    torch.cuda.synchronize()
    _guards_intact(_lid(case) + " y", ybuf, M)
    _guards_intact(_lid(case) + " x", xbuf, M)
    xr = x[:M] + te[(torch.arange(M, device=dev) // T) % F] if use_te else x[:M]
    assert _same_bits(xin, xr), "the fp32 x written back is not torch's fp32 add"
    want, bound, mag = ln_expected(case, xr, mod)
    ratio = worst(_lid(case), y, want, bound)
    print(f"ln_modulate {_lid(case)}: worst err / bound {ratio:.3f}, {_half_ulps(y, want, mag, dt)}")
