"""Text cross-attention (csrc/attention.hip: launch_cross_attention) by itself, through latte_debug_cross_attention: the whole-panel
kernel attn_cross_kernel (Lk <= 128 and L >= 128) and the CROSS form of attn_flash_kernel (everything else, and everything under
latte_debug_set_choice("xattn_flash", 1)), per element against

    want = softmax(q k^T hd^-1/2 + bias) v      in fp64, on the same half-rounded q, k, v,

indexed as the engine does: sample = seq // U, the keys of sample s at rows [s Lk, (s + 1) Lk) of kv [B Lk, 2 D] = [K | V].

THE BOUND (per output element, first order, nothing in it measured on a GPU).  Both kernels work in the exp2 domain:
z_k = s_k c + b_k, s_k = q . k_k (MFMA, fp32 accumulation of hd products), c = hd^-1/2 log2(e), b_k = bias_k log2(e); p~_k = exp2(z_k - m);
l = sum_k p~_k in fp32; P~ = half(p~); o = sum_k P~_k v_k (MFMA, fp32); out = half(o / l).  With P_k = p_k / l the exact probabilities,
u the unit roundoff of the half type (2^-11 f16, 2^-8 bf16) and e = 2^-24 that of fp32:

  output rounding          u |out|  <=  u |want| + u (everything below); f16: + 2^-25, the rounding of a subnormal result
  P~ = half(p~)            u sum_k P_k |v_k|; f16: + 2^-25 sum_k |v_k| / l for the p~ that land among the subnormals (l >= 1: p~_max = 1)
  score and exponential    a score error dz_k changes p_k by the factor 2^dz_k: relative ln2 dz_k, and the common part of dz cancels
                           between p~ and l.  dz_k <= e ((hd + 4) c sum_i |q_i k_ki| + 2 |b_k| + |z_k| + 2 |z_k - m|): the hd products
                           of the chain, the three roundings inside c and the product s c; the two roundings of b_k; the rounding of
                           the sum z_k; the subtraction z_k - m and, in the flash form, the running-maximum rescales a key's term
                           goes through, whose exponents telescope to at most m - z_k.  exp2 itself: one ulp = 2 e, each of the nt
                           rescales of the flash form 3 e more (nt = ceil(Lk / 64) key tiles).  Together rho_k = ln2 dz_k + (2 + 3 nt) e
                           and the term  sum_k P_k rho_k |v_k| + |want| sum_k P_k rho_k  (numerator and denominator).
  fully masked rows        every key of the sample carries the bias -10000: b_k is the SAME rounded product for every key and cancels,
                           but z_k = s_k c + b_k is rounded at magnitude 10000 log2(e) = 14427, where one fp32 ulp is 2^-10 in the exp2
                           domain: once in the panel kernel (one fma), twice in the flash form (product, then sum).  For these rows
                           dz_k = e ((hd + 4) c sum_i |q_i k_ki| + 2 |z_k - m|) + {1, 2} x 2^-10.
  the two fp32 sums        l: Lk additions, relative to |want|; o: Lk products, relative to sum_k P_k |v_k|; plus the nt rescales and the
                           reciprocal and product of the normalisation:  e ((Lk + nt) sum_k P_k |v_k| + (Lk + nt + 2) |want|).

A masked key of a sample that keeps at least one key has z_k - m <= -14000: exp2 returns exactly 0 (as exp does in the fp64 reference), so
its K and V rows cannot reach the output at all -- checked without a tolerance, like everything else that must not be read: the columns
beyond D of a q row (q_ld = 3 D), the rows behind the last query and behind the last sample's keys (all NaN), the other sample's keys
and bias.  `out` is NaN before every launch and sits between guard rows that must come back bit for bit.

Worst err / bound over every case, form and mask on the MI355X: 0.860 (Lk = 7, bf16)."""
import math

import pytest
import torch

from latte_amd._lib import check, ptr, stream_ptr

pytestmark = pytest.mark.gpu

TD = {"bf16": torch.bfloat16, "f16": torch.float16}
DT = {"bf16": 0, "f16": 1}
U_HALF = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11}    # unit roundoff of the half type
ETA = {"bf16": 0.0, "f16": 2.0 ** -25}             # absolute rounding error among the f16 subnormals
U32 = 2.0 ** -24
LOG2E = 1.4426950408889634
LN2 = math.log(2.0)
ULP_MASKED = 2.0 ** -10                            # one fp32 ulp at 10000 log2(e) = 14427 (in [2^13, 2^14): 2^(13 - 23))
HEADS, B = 2, 2
GUARD = 3                                          # guard rows around out, behind q and behind kv
SENT = -7.25
MASKS = ["none", "ones", "pattern", "sample1_masked", "key0_only", "normal"]


def _cases():
    """(hd, dt, U, L, Lk, q_ld multiple, layout).  Every Lk <= 128 meets an L >= 128 (both forms run), every L >= 128 an Lk <= 128; Lk
    129 and 200 and L = 64 are flash only.  Each value of L, Lk, U and q_ld appears under each of the four (hd, dtype) pairs, with the
    pairing rotated from one to the next.  layout 0: a sequence is L consecutive rows (spatial), 1: rows U apart (temporal addressing)."""
    out = []
    for ci, (hd, dt) in enumerate([(64, "bf16"), (64, "f16"), (72, "bf16"), (72, "f16")]):
        for i, Lk in enumerate([1, 7, 33, 64, 65, 120, 128]):
            out.append((hd, dt, 3 + (i + ci) % 2, [128, 144, 256, 300][(i + ci) % 4], Lk, 1 + 2 * ((i + ci // 2) % 2), (i // 2 + ci) % 2))
        out.append((hd, dt, 3 + ci % 2, 64, 129, 1 + 2 * (ci % 2), 0))
        out.append((hd, dt, 4 - ci % 2, [144, 300][ci % 2], 200, 3 - 2 * (ci % 2), 1))
        out.append((hd, dt, 4 - ci % 2, 64, [33, 120][ci % 2], 3 - 2 * (ci % 2), ci % 2))   # L = 64 with few keys: flash by the L rule
    return out


CASES = _cases()


def _id(c):
    hd, dt, U, L, Lk, qm, lay = c
    return f"hd{hd}-{dt}-U{U}-L{L}-Lk{Lk}-qld{qm}D-lay{lay}"


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


def _choice(lib, value):
    check(lib.latte_debug_set_choice(b"xattn_flash", value))


def _bits(t):
    return t.contiguous().view(torch.int16)


class Shape:
    """The buffers of one case.  q [rows + GUARD, q_ld]: columns >= D and the guard rows are NaN; kv [B Lk + GUARD, 2 D]: guard rows NaN;
    out [GUARD + rows + GUARD, D]."""
    def __init__(self, case, dev, g):
        hd, dt, U, L, Lk, qm, lay = case
        self.hd, self.dt, self.U, self.L, self.Lk, self.dev = hd, dt, U, L, Lk, dev
        self.D = D = HEADS * hd
        self.q_ld = qm * D
        self.S = S = B * U
        self.rows = rows = S * L
        self.sample_stride = U * L
        self.seq_stride, self.row_stride = (L, 1) if lay == 0 else (1, U)
        seq = torch.arange(S, device=dev)
        self.row_of = ((seq // U) * self.sample_stride + (seq % U) * self.seq_stride)[:, None] + torch.arange(L, device=dev)[None, :] * self.row_stride
        assert sorted(self.row_of.flatten().tolist()) == list(range(rows))
        self.q = torch.full((rows + GUARD, self.q_ld), float("nan"), device=dev, dtype=TD[dt])
        self.q[:rows, :D] = torch.randn(rows, D, generator=g, device=dev).to(TD[dt])
        self.kv = torch.full((B * Lk + GUARD, 2 * D), float("nan"), device=dev, dtype=TD[dt])
        self.kv[:B * Lk] = torch.randn(B * Lk, 2 * D, generator=g, device=dev).to(TD[dt])
        self.out = torch.empty(rows + 2 * GUARD, D, device=dev, dtype=TD[dt])
        self.bias = torch.empty(B * Lk + GUARD, device=dev)
        self.smp_of_seq = seq // U

    def mask(self, kind, g):
        """-> the 0/1 mask [B, Lk] of a pattern (None: no bias; "normal": a real-valued bias instead of a mask)."""
        Lk, dev = self.Lk, self.dev
        k = torch.arange(Lk, device=dev)
        m = torch.ones(B, Lk, device=dev)
        if kind == "pattern":                      # trailing third masked on sample 0, interior holes on sample 1
            m[0, k >= Lk - Lk // 3] = 0.0
            m[1, (k % 3 == 1) & (k < Lk - 1)] = 0.0
        elif kind == "sample1_masked":
            m[1] = 0.0
        elif kind == "key0_only":
            m[:, 1:] = 0.0
        return m

    def set_bias(self, lib, kind, g):
        """Fills self.bias for a mask kind through latte_debug_mask_bias (checked bit for bit against torch fp32); -> the bias tensor
        to pass (None for "none") and its [B, Lk] values."""
        n = B * self.Lk
        self.bias.fill_(float("nan"))
        if kind == "none":
            return None, None
        if kind == "normal":
            self.bias[:n] = torch.randn(n, generator=g, device=self.dev)
        else:
            m = self.mask(kind, g)
            _call(lib, "latte_debug_mask_bias", m, self.bias, n)
            _sync(self.dev)
            assert torch.equal(self.bias[:n].view(torch.int32), ((1.0 - m.flatten()) * -10000.0).view(torch.int32)), "mask_bias"
            assert bool(torch.isnan(self.bias[n:]).all()), "mask_bias wrote past n"
        return self.bias, self.bias[:n].view(B, self.Lk).clone()

    def run(self, lib, bias, flash):
        """One launch into a NaN-prefilled out between sentinel guard rows; -> the [S, L, D] result in sequence order."""
        self.out.fill_(float("nan"))
        self.out[:GUARD] = SENT
        self.out[GUARD + self.rows:] = SENT
        _choice(lib, 1 if flash else 0)
        try:
            _call(lib, "latte_debug_cross_attention", self.q, self.q_ld, self.kv, bias, self.out[GUARD:], self.S, self.L, self.Lk, HEADS,
                  self.hd, self.U, self.sample_stride, self.seq_stride, self.row_stride, DT[self.dt])
            _sync(self.dev)
        finally:
            _choice(lib, 0)
        sent = torch.full((GUARD, self.D), SENT, device=self.dev, dtype=TD[self.dt])
        assert torch.equal(_bits(self.out[:GUARD]), _bits(sent)), "wrote in front of out"
        assert torch.equal(_bits(self.out[GUARD + self.rows:]), _bits(sent)), "wrote behind out"
        got = self.out[GUARD:GUARD + self.rows][self.row_of]             # [S, L, D]
        bad = ~torch.isfinite(got).all(-1)
        assert not bool(bad.any()), (f"{int(bad.sum())} rows not finite (unwritten, or NaN read from a guard); first (seq, token) "
                                     f"{tuple(int(i) for i in torch.nonzero(bad)[0])}")
        return got

    def reference(self, bias_bl):
        """fp64 want [S, L, D] and the per-form bounds {False: panel, True: flash} of the module docstring."""
        hd, Lk, D, S, L = self.hd, self.Lk, self.D, self.S, self.L
        q = self.q[:self.rows, :D][self.row_of].double().view(S, L, HEADS, hd).permute(0, 2, 1, 3)            # [S, H, L, hd]
        kvs = self.kv[:B * Lk].double().view(B, Lk, 2, HEADS, hd)[self.smp_of_seq]                              # [S, Lk, 2, H, hd]
        k, v = kvs[:, :, 0].permute(0, 2, 1, 3), kvs[:, :, 1].permute(0, 2, 1, 3)                              # [S, H, Lk, hd]
        c = hd ** -0.5 * LOG2E
        s_abs = q.abs() @ k.abs().transpose(-1, -2)
        bz = torch.zeros(S, 1, 1, Lk, device=self.dev, dtype=torch.float64)
        all_masked = torch.zeros(S, dtype=torch.bool, device=self.dev)
        if bias_bl is not None:
            bz = (bias_bl.double() * LOG2E)[self.smp_of_seq][:, None, None, :]
            all_masked = (bias_bl == -10000.0).all(-1)[self.smp_of_seq]
        z = (q @ k.transpose(-1, -2)) * c + bz
        m = z.max(-1, keepdim=True).values
        p = torch.exp2(z - m)
        l = p.sum(-1, keepdim=True)
        P = p / l
        want = P @ v
        pv_abs = P @ v.abs()
        v_abs_sum = v.abs().sum(-2, keepdim=True)                                                               # [S, H, 1, hd]
        nt = (Lk + 63) // 64
        am = all_masked[:, None, None, None]
        bounds = {}
        for flash in (False, True):
            dz_plain = U32 * ((hd + 4) * c * s_abs + 2 * bz.abs() + z.abs() + 2 * (z - m).abs())
            dz_masked = U32 * ((hd + 4) * c * s_abs + 2 * (z - m).abs()) + (2 if flash else 1) * ULP_MASKED
            rho = LN2 * torch.where(am, dz_masked, dz_plain) + (2 + 3 * nt) * U32
            e_score = (P * rho) @ v.abs() + want.abs() * (P * rho).sum(-1, keepdim=True)
            e_sums = U32 * ((Lk + nt) * pv_abs + (Lk + nt + 2) * want.abs())
            e_half = U_HALF[self.dt] * pv_abs + ETA[self.dt] * v_abs_sum / l
            bound = (e_score + e_sums + e_half) * (1 + U_HALF[self.dt]) + U_HALF[self.dt] * want.abs() + ETA[self.dt]
            bounds[flash] = bound.permute(0, 2, 1, 3).reshape(S, L, D)
        return want.permute(0, 2, 1, 3).reshape(S, L, D), bounds, all_masked


def _check(tag, got, want, bound, seqs=None):
    err = (got.double() - want).abs()
    bad = ~(err <= bound)
    if seqs is not None:
        bad = bad & seqs[:, None, None]
    ratio = float((err / bound).max())
    if bool(bad.any()):
        i = tuple(int(x) for x in torch.nonzero(bad)[0])
        raise AssertionError(f"{tag}: {int(bad.sum())} of {err.numel()} elements out of bound; first (seq, token, column) {i}: got "
                             f"{float(got[i]):.6e} want {float(want[i]):.6e} err {float(err[i]):.3e} > {float(bound[i]):.3e}; worst err / bound {ratio:.3f}")
    return ratio


def _same_bits(tag, a, b, seqs):
    ne = (_bits(a) != _bits(b)).any(-1).any(-1) & seqs
    assert not bool(ne.any()), f"{tag}: sequences {[int(i) for i in torch.nonzero(ne).flatten()]} changed"


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_cross_attention(lib, dev, case):
    hd, dt, U, L, Lk, qm, lay = case
    g = torch.Generator(dev).manual_seed(1000 * Lk + L + hd + DT[dt])
    sh = Shape(case, dev, g)
    forms = [False, True] if (Lk <= 128 and L >= 128) else [True]       # False: the launcher's own choice, here the panel kernel
    n = B * Lk
    kv0 = sh.kv.clone()
    other = torch.randn(n, 2 * sh.D, generator=g, device=dev).to(TD[dt])          # the "other finite values" of the bit checks
    s0 = sh.smp_of_seq == 0
    worst = 0.0
    for kind in MASKS:
        bias, bias_bl = sh.set_bias(lib, kind, g)
        want, bounds, all_masked = sh.reference(bias_bl)
        got = {}
        for flash in forms:
            tag = f"{_id(case)} mask {kind} {'flash' if flash else 'panel'}"
            got[flash] = sh.run(lib, bias, flash)
            worst = max(worst, _check(tag, got[flash], want, bounds[flash]))
            if kind in ("pattern", "key0_only"):
                # masked keys of a sample that keeps a key: other K / V rows there, same bits (a fully masked sample keeps its rows)
                keeps = (bias_bl == 0.0).any(-1)
                repl = ((bias_bl == -10000.0) & keeps[:, None]).flatten()
                sh.kv[:n] = torch.where(repl[:, None], other, kv0[:n])
                _same_bits(tag + ": K / V rows of masked keys replaced", sh.run(lib, bias, flash), got[flash],
                           torch.ones_like(s0))
                sh.kv.copy_(kv0)
            if kind == "pattern":
                # sample isolation: sample 1's keys, values and bias replaced, sample 0 must not move (Lk = 1, 65, 120: the staged
                # images re-read row Lk - 1 of sample 0, the row in front of sample 1's first)
                sh.kv[Lk:n] = other[Lk:n]
                sh.bias[Lk:n] = -10000.0 * (torch.rand(Lk, generator=g, device=dev) < 0.5)
                _same_bits(tag + ": sample 1 replaced", sh.run(lib, bias, flash), got[flash], s0)
                sh.kv.copy_(kv0)
                sh.bias[:n] = bias_bl.flatten()
        if len(forms) == 2:
            _check(f"{_id(case)} mask {kind} panel against flash", got[False], got[True].double(), bounds[False] + bounds[True])
    print(f"{_id(case)}: worst err / bound {worst:.3f}")


def test_cross_attention_hook_refuses(lib, dev):
    """What launch_cross_attention assumes and the hook checks: q_ld >= D, 16-byte rows, head dim 64 | 72, positive sizes."""
    hd, L, Lk, U = 64, 64, 7, 3
    D = HEADS * hd
    q = torch.zeros(B * U * L, 3 * D, device=dev, dtype=torch.float16)
    kv = torch.zeros(B * Lk, 2 * D, device=dev, dtype=torch.float16)
    out = torch.zeros(B * U * L, D, device=dev, dtype=torch.float16)

    def rc(q_ld=D, hd_=hd, L_=L, Lk_=Lk, U_=U, kv_=kv):
        return lib.latte_debug_cross_attention(ptr(q), q_ld, ptr(kv_), ptr(None), ptr(out), B * U, L_, Lk_, HEADS, hd_, U_, U * L, L, 1, 1,
                                               stream_ptr())
    assert rc() == 0
    _sync(dev)
    for kw in (dict(q_ld=D - 8), dict(q_ld=D + 4), dict(hd_=80), dict(L_=0), dict(Lk_=0), dict(U_=0), dict(kv_=None)):
        assert rc(**kw) == 1, kw
