"""Self-attention (csrc/attention.hip: launch_attention) by itself, through latte_debug_attention: the six kernels behind the launcher --
attn_small (L <= 16), the generic flash kernel (16 < L <= 128, and everything under attn_variant 1), attn_full (128 < L <= 256),
attn_stream (L > 256, and 128 < L under attn_variant 5), attn_stream64 in its 4-wave and 8-wave forms (attn_variant 12 / 13, head dim
72 and L > 256) -- per element against

    want = softmax(q k^T hd^-1/2) v      in fp64, on the same half-rounded q, k, v,

read out of a [rows, 3 D] buffer in the column order [3][heads][hd], a sequence addressed as the engine does: base row
(seq / U) sample_stride + (seq % U) seq_stride, token t at base + t row_stride.  Both addressings run: a sequence as L consecutive rows
(seq_stride L, row_stride 1) and as rows U apart (seq_stride 1, row_stride U).

THE BOUND (per output element, first order, nothing in it measured on a GPU).  It is the chain of tests/test_cross_attention.py without
the bias terms; every kernel works in the exp2 domain with c = hd^-1/2 log2(e): z_k = s_k c, s_k = q . k_k (MFMA, fp32 accumulation of hd
products), p~_k = exp2(z_k - m~), m~ the reference maximum the kernel holds when it meets key k, l = sum_k p~_k in fp32, P~ = half(p~),
o = sum_k P~_k v_k (MFMA, fp32), out = half(o / l).  With P_k the exact probabilities, m = max_k z_k, u the unit roundoff of the half type
(2^-11 f16, 2^-8 bf16), e = 2^-24 and nt the kernel's own number of key blocks (attn_small and attn_full: 1; flash and attn_stream64:
ceil(L / 64); attn_stream: ceil(L / 128)):

  output rounding          u |out|  <=  u |want| + u (everything below); f16: + 2^-25, the rounding of a subnormal result
                           (store_out4: pack2 of o[d][r] * inv)
  P~ = half(p~)            u sum_k P_k |v_k|; f16: + 2^-25 sum_k |v_k| / l for the p~ that land among the subnormals (l >= 1: the key
                           that set the reference maximum has p~ = 1).  Every kernel rounds P: pack2 in front of the PV MFMA -- attn_small
                           too (attention.hip: `pb = {pack2(st[0], st[1]), ...}`).
  score and exponential    a score error dz_k changes p_k by the factor 2^dz_k: relative ln2 dz_k.  dz_k <= e ((hd + 4) c sum_i |q_i k_ki|
                           + max(|z_k|, |m|) + 2 |z_k - m|):
                             the hd products of the MFMA chain, the three roundings inside c and the product with c;
                             flash: z = st * c is rounded at |z_k|; full / stream / stream64 / small: nm = -m~ c is rounded at |m~ c|,
                             and m~ lies between z_k and m -- within one block that error is common to p~ and l and cancels, across blocks
                             it is not, so it is counted: max(|z_k|, |m|);
                             the subtraction z_k - m~ (flash) or the one rounding of fma(s, c, nm) (the others), at most |z_k - m|;
                             the rescales alpha = exp2(m_old - m_new) [flash] or exp2((m_old - m_new) c) [stream: one subtraction and one
                             product] a key's term goes through: their exponents telescope to at most m - z_k, once more |z_k - m|.
                           exp2 itself: one ulp = 2 e; each of the nt rescales 3 e more (exp2 and the product).  Together
                           rho_k = ln2 dz_k + (2 + 3 nt) e and the term  sum_k P_k rho_k |v_k| + |want| sum_k P_k rho_k.
  attn_stream64, LAZY = 8  the reference maximum is raised only when some query of the 32-query group finds a score more than 2^8 (in the
                           exp2 domain) above its own; until then p~_k <= 2^8.  half(p~) keeps the SAME relative rounding u (256 is far
                           below the f16 maximum 65504 and l <= 256 L is far below the fp32 one: no overflow), and the f16 subnormal term
                           does not grow: the reference m~ is itself one of the scores, its key has p~ = 1, so l >= 1 as before and the l
                           of the bound -- taken at the true maximum -- is the smaller one.  What changes is the size of the rounded
                           quantities: |m~ c| <= max(|z_k|, |m|) + 8, |z_k - m~| <= |z_k - m| + 8 and the telescoped rescales
                           <= |z_k - m| + 8: dz_k grows by 3 x 8 e.
  the two fp32 sums        l: L additions, relative to |want|; o: L products, relative to sum_k P_k |v_k|; plus the nt rescales and the
                           reciprocal (1.0f / l: a correctly rounded division in this build) and product of the normalisation:
                           e ((L + nt) sum_k P_k |v_k| + (L + nt + 2) |want|).
  (v_exp_f32 flushes results below 2^-126 to zero: an absolute 2^-126 per key, far below every other term.)

INPUTS.  q of (sequence, head) is scaled so that the scores q k^T hd^-1/2 have the standard deviation 1/4, 1 or 4 (near-uniform to peaked
rows); V has a per-column offset of up to 4 sigma, so a dropped key or a wrong normaliser moves every element; for L > 128 key L - 2 (in
the LAST key block) dominates query 5 and key 10 dominates the last query (a later query block): the forced rescales.

WITHOUT A TOLERANCE.  `out` is NaN before every launch and lies between guard rows that must come back bit for bit; the rows behind the
last sequence are NaN in qkv; the same launch twice gives the same bits; sample 1's rows replaced, sample 0's output keeps its bits.
launch_attention's `stream_ok` refuses nothing: where 128 rows of a block span 2 GiB or more it runs the generic flash kernel instead.
That needs row_stride D > 2^31 / 768, a qkv buffer of more than 4 GiB at L = 257 -- not reached here; every shape below is accepted under
both addressings, which test_every_shape_is_accepted_under_both_addressings states.

The CPU half (not marked gpu) runs a torch stand-in that rounds where the kernels round (exp2 domain, l in fp32, P~ = half(p~), block-wise
rescale, the lazy maximum) through the same bound on the same cases, and shows that five named mistakes leave it.

Worst err / bound per kernel on the MI355X: DESIGN.md section 4.11."""
import math

import pytest
import torch

gpu = pytest.mark.gpu
TD = {"bf16": torch.bfloat16, "f16": torch.float16}
DT = {"bf16": 0, "f16": 1}
U_HALF = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11}
ETA = {"bf16": 0.0, "f16": 2.0 ** -25}
U32 = 2.0 ** -24
LOG2E = 1.4426950408889634
LN2 = math.log(2.0)
LAZY = 8.0
B = 2
GUARD = 3
SENT = -7.25
NEG_BIG = -1.0e30

# kernel -> (attn_variant, keys per block (0: the whole sequence), queries per workgroup, lazy maximum, the L it is reached at)
KERNELS = {
    "small": (0, 0, 16, False, [1, 2, 5, 16]),
    "flash": (0, 64, 64, False, [17, 64, 65, 100, 128]),
    "flash_forced": (1, 64, 64, False, [129, 300]),
    "full": (0, 0, 256, False, [129, 200, 256]),
    "stream": (0, 128, 256, False, [257, 300, 513, 1024]),
    "stream_forced": (5, 128, 256, False, [129, 200, 256]),
    "stream64": (12, 64, 256, True, [300, 513, 1024]),
    "stream64_8w": (13, 64, 256, True, [300, 513, 1024]),
}


def _cases():
    """(kernel, L, hd, dt, heads, U, layout): every (kernel, L) under each (hd, dtype) pair the kernel exists for, heads, U and the
    addressing rotated from one to the next, so that each (kernel, L) meets both addressings.  layout 0: a sequence is L consecutive
    rows, 1: rows U apart."""
    out = []
    for kernel, (variant, kb, qb, lazy, Ls) in KERNELS.items():
        pairs = [(72, "bf16"), (72, "f16")] if lazy else [(64, "bf16"), (64, "f16"), (72, "bf16"), (72, "f16")]
        for i, L in enumerate(Ls):
            for ci, (hd, dt) in enumerate(pairs):
                out.append((kernel, L, hd, dt, 2 + (i + ci // 2) % 2, 2 + (i + ci + 1) % 2, (i + ci) % 2))
    return out


CASES = _cases()


def _id(c):
    kernel, L, hd, dt, H, U, lay = c
    return f"{kernel}-L{L}-hd{hd}-{dt}-H{H}-U{U}-lay{lay}"


def n_blocks(kernel, L):
    kb = KERNELS[kernel][1]
    return 1 if kb == 0 else -(-L // kb)


def row_map(L, U, lay, dev, swap=False):
    """-> (row_of [S, L], sample_stride, seq_stride, row_stride); swap: the two strides exchanged (a named mistake; rows wrap)."""
    S = B * U
    seq_stride, row_stride = (L, 1) if lay == 0 else (1, U)
    if swap:
        seq_stride, row_stride = row_stride, seq_stride
    seq = torch.arange(S, device=dev)
    row_of = ((seq // U) * (U * L) + (seq % U) * seq_stride)[:, None] + torch.arange(L, device=dev)[None, :] * row_stride
    return row_of % (S * L), U * L, seq_stride, row_stride


def make_inputs(case, dev, seed_shift=0):
    """-> x [S, L, 3, H, hd] of the half type (module docstring: INPUTS)"""
    kernel, L, hd, dt, H, U, lay = case
    S = B * U
    g = torch.Generator(dev).manual_seed(1000 * L + hd + DT[dt] + 7 * H + seed_shift)
    x = torch.randn(S, L, 3, H, hd, generator=g, device=dev)
    sig = torch.tensor([0.25, 1.0, 4.0], device=dev)[(torch.arange(S, device=dev)[:, None] + torch.arange(H, device=dev)[None, :]) % 3]   # [S, H]
    x[:, :, 0] *= sig[:, None, :, None]
    x[:, :, 2] += torch.rand(S, 1, H, hd, generator=g, device=dev) * 8 - 4
    if L > 128:
        x[:, L - 2, 1] = x[:, 5, 0] * 6.0 / sig[:, :, None] ** 2          # a key of the LAST block dominates an early query
        x[:, 10, 1] = x[:, L - 1, 0] * 5.0 / sig[:, :, None] ** 2         # an early key dominates the last query
    return x.to(TD[dt])


def pack_rows(x, row_of):
    """x [S, L, 3, H, hd] -> qkv [rows + GUARD, 3 D], the guard rows NaN"""
    S, L = x.shape[:2]
    qkv = torch.full((S * L + GUARD, x[0, 0].numel()), float("nan"), device=x.device, dtype=x.dtype)
    qkv[row_of] = x.reshape(S, L, -1)
    return qkv


# ------------------------------------------------------------------------------------------------ fp64 reference and bound
def reference(x, kernel):
    """x [S, L, 3, H, hd] half -> (want, bound), fp64 [S, L, H hd] (module docstring)"""
    S, L, _, H, hd = x.shape
    dt = "bf16" if x.dtype == torch.bfloat16 else "f16"
    q, k, v = (x[:, :, i].double().permute(0, 2, 1, 3) for i in range(3))                      # [S, H, L, hd]
    c = hd ** -0.5 * LOG2E
    s_abs = q.abs() @ k.abs().transpose(-1, -2)
    z = (q @ k.transpose(-1, -2)) * c
    m = z.max(-1, keepdim=True).values
    p = torch.exp2(z - m)
    l = p.sum(-1, keepdim=True)
    P = p / l
    want = P @ v
    pv_abs = P @ v.abs()
    v_abs_sum = v.abs().sum(-2, keepdim=True)
    nt = n_blocks(kernel, L)
    lazy = LAZY if KERNELS[kernel][3] else 0.0
    dz = U32 * ((hd + 4) * c * s_abs + torch.maximum(z.abs(), m.abs()) + 2 * (z - m).abs() + 3 * lazy)
    rho = LN2 * dz + (2 + 3 * nt) * U32
    e_score = (P * rho) @ v.abs() + want.abs() * (P * rho).sum(-1, keepdim=True)
    e_sums = U32 * ((L + nt) * pv_abs + (L + nt + 2) * want.abs())
    e_half = U_HALF[dt] * pv_abs + ETA[dt] * v_abs_sum / l
    bound = (e_score + e_sums + e_half) * (1 + U_HALF[dt]) + U_HALF[dt] * want.abs() + ETA[dt]
    return want.permute(0, 2, 1, 3).reshape(S, L, H * hd), bound.permute(0, 2, 1, 3).reshape(S, L, H * hd)


def worst(tag, got, want, bound, raise_=True):
    """-> worst err / bound; an element that is not finite counts as out of bound"""
    err = (got.double() - want).abs()
    bad = ~(err <= bound)
    ratio = float(torch.nan_to_num(err / bound, nan=float("inf")).max())
    if raise_ and bool(bad.any()):
        i = tuple(int(t) for t in torch.nonzero(bad)[0])
        raise AssertionError(f"{tag}: {int(bad.sum())} of {err.numel()} elements out of bound; first (seq, token, column) {i}: got "
                             f"{float(got[i]):.6e} want {float(want[i]):.6e} err {float(err[i]):.3e} > {float(bound[i]):.3e}; worst err / bound {ratio:.3f}")
    return ratio


# ------------------------------------------------------------------------------------------------ the kernels restated in fp32
MISTAKES = ("last_key_dropped", "alpha_one", "head_at_64h", "strides_swapped", "last_query_block")


def _fma(a, b, c):
    return (a.double() * b.double() + c.double()).float()


def standin(qkv, case, mistake=None, drop_for=None):
    """The kernel of `case` in torch fp32 on the packed buffer -> out [S, L, D] of the half type (NaN where nothing is written).
    Per key block: scores in fp32; the flash kernel scales them first (z = s c, maximum and exponent on z), the others keep the maximum
    on the raw scores and form exp2(fma(s, c, -m c)); alpha, l = l alpha + sum p~ in fp32; o = o alpha + half(p~) v; out = half(o / l).
    drop_for = (seq, head, first query): `last_key_dropped` for that 64-query block whatever the raggedness (default: the last sequence
    and head, queries 0..63, and only where the last key block is ragged)."""
    kernel, L, hd, dt, H, U, lay = case
    variant, kb, qb, lazy, _ = KERNELS[kernel]
    kb = kb or L
    S, D = B * U, H * hd
    dev = qkv.device
    row_of, _, _, _ = row_map(L, U, lay, dev, swap=mistake == "strides_swapped")
    rows = qkv[:S * L][row_of].float()                                                         # [S, L, 3 D]
    col0 = (64 if (mistake == "head_at_64h" and hd == 72) else hd) * torch.arange(H, device=dev)
    cols = col0[:, None] + torch.arange(hd, device=dev)[None, :]                              # [H, hd]
    q, k, v = (rows[:, :, i * D + cols].permute(0, 2, 1, 3) for i in range(3))                # [S, H, L, hd]
    c = torch.tensor(hd, dtype=torch.float32).rsqrt() * torch.tensor(LOG2E, dtype=torch.float32)
    flash = kernel.startswith("flash")
    m_run = torch.full((S, H, L, 1), NEG_BIG)
    l_run = torch.zeros(S, H, L, 1)
    o = torch.zeros(S, H, L, hd)
    for k0 in range(0, L, kb):
        kk, vv = k[:, :, k0:k0 + kb], v[:, :, k0:k0 + kb]
        s = q @ kk.transpose(-1, -2)
        if mistake == "last_key_dropped" and k0 + kb >= L and (drop_for is not None or L % (KERNELS[kernel][1] or 256)):
            sq, hq, q0 = drop_for or (S - 1, H - 1, 0)
            s[sq, hq, q0:q0 + 64, -1] = NEG_BIG
        if flash:
            s = s * c
        mx = s.max(-1, keepdim=True).values
        if lazy:        # raised for a 32-query group when any of its queries finds a score more than LAZY above its reference
            over = ((mx - m_run) * c > LAZY).float()
            pad = (-L) % 32
            up = torch.nn.functional.pad(over, (0, 0, 0, pad)).view(S, H, -1, 32, 1).amax(3, keepdim=True).expand(-1, -1, -1, 32, -1).reshape(S, H, -1, 1)[:, :, :L] > 0
            m_new = torch.where(up, torch.maximum(m_run, mx), m_run)
        else:
            m_new = torch.maximum(m_run, mx)
        if flash:
            alpha = torch.exp2(m_run - m_new)
            p = torch.exp2(s - m_new)
        else:
            alpha = torch.exp2((m_run - m_new) * c)
            p = torch.exp2(_fma(s, c, -m_new * c))
        if mistake == "alpha_one" and k0 > 0:
            alpha = torch.ones_like(alpha)
        l_run = l_run * alpha + p.sum(-1, keepdim=True)
        o = o * alpha + p.to(TD[dt]).float() @ vv
        m_run = m_new
    out = (o * (1.0 / l_run)).to(TD[dt]).permute(0, 2, 1, 3).reshape(S, L, D)
    if mistake == "last_query_block" and L % qb:
        out[:, L // qb * qb:] = float("nan")
    return out


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_standin_within_bound(case):
    """the restated kernel passes what the GPU result has to pass"""
    kernel, L, hd, dt, H, U, lay = case
    dev = torch.device("cpu")
    x = make_inputs(case, dev)
    want, bound = reference(x, kernel)
    got = standin(pack_rows(x, row_map(L, U, lay, dev)[0]), case)
    ratio = worst(_id(case), got, want, bound)
    assert ratio < 1.0
    print(f"stand-in {_id(case)}: worst err / bound {ratio:.3f}")


def _applies(case, mistake):
    kernel, L, hd, dt, H, U, lay = case
    variant, kb, qb, lazy, _ = KERNELS[kernel]
    return {"last_key_dropped": L % (kb or 256) != 0, "alpha_one": kb != 0 and L > kb, "head_at_64h": hd == 72, "strides_swapped": L > 1,
            "last_query_block": L % qb != 0}[mistake]


@pytest.mark.parametrize("mistake", MISTAKES)
def test_named_mistakes_leave_the_bound(mistake):
    """One mistake at a time over the cases it can show in (one (hd, dtype) pair per (kernel, L) to keep it short): at least one fails.
    Failing / tried, as run on the CPU: last_key_dropped 20 / 20, alpha_one 18 / 18, head_at_64h 27 / 27, strides_swapped 26 / 26,
    last_query_block 19 / 19."""
    dev = torch.device("cpu")
    seen, tried, failed = set(), 0, []
    for case in CASES:
        kernel, L, hd, dt, H, U, lay = case
        if not _applies(case, mistake) or (kernel, L) in seen:
            continue
        seen.add((kernel, L))
        x = make_inputs(case, dev)
        want, bound = reference(x, kernel)
        got = standin(pack_rows(x, row_map(L, U, lay, dev)[0]), case, mistake)
        tried += 1
        if worst("", got, want, bound, raise_=False) > 1.0:
            failed.append(_id(case))
    print(f"{mistake}: {len(failed)} of {tried} cases fail")
    assert failed, mistake


@pytest.mark.parametrize("shape,dt,tol", [((1, 2, 1024, 2, 72), "bf16", 8e-3), ((2, 16, 256, 16, 72), "f16", 1.5e-3)])
def test_dropped_last_key_passes_the_norm_wise_test(shape, dt, tol):
    """Why this file exists: 64 queries of one head ignoring the last key stay under the tolerance of test_gpu_kernels.test_attention
    (its seed, its N(0, 1) inputs, its whole-tensor ratio against fp32 softmax) and leave the per-element bound."""
    Bv, F, T, H, hd = shape
    rows, D = Bv * F * T, H * hd
    g = torch.Generator("cpu").manual_seed(rows + hd)
    qh = torch.randn(rows, 3 * D, generator=g).to(TD[dt])
    S = Bv * F
    S = min(S, 2)               # two sequences are restated; the others enter the whole-tensor ratio below with the clean pair's
                                # squared error and norm (same distribution, no mistake in them)
    x = qh[:S * T].view(S, T, 3, H, hd)
    case = ("stream" if T > 256 else "full", T, hd, dt, H, S // B, 0)
    qkv = pack_rows(x, row_map(T, S // B, 0, torch.device("cpu"))[0])
    want, bound = reference(x, case[0])
    good = standin(qkv, case)
    bad = standin(qkv, case, "last_key_dropped", drop_for=(0, 0, 0))      # whatever the raggedness
    xf = x.float()
    q, k, v = (xf[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    ref32 = (torch.softmax((q @ k.transpose(-1, -2)) * hd ** -0.5, -1) @ v).permute(0, 2, 1, 3).reshape(S, T, D)
    scale = (Bv * F) / S
    clean = float((good.float() - ref32).norm() / ref32.norm())
    num2 = float((bad.float() - ref32).norm()) ** 2 + (scale - 1) * float((good.float() - ref32).norm()) ** 2
    rel = math.sqrt(num2 / (scale * float(ref32.norm()) ** 2))
    print(f"{shape} {dt}: clean {clean:.2e}, with the mistake {rel:.2e}, tolerance {tol:.1e}")
    assert rel < tol
    assert worst("", good, want, bound, raise_=False) < 1.0
    assert worst("", bad, want, bound, raise_=False) > 1.0


def test_every_shape_is_accepted_under_both_addressings():
    """stream_ok (launch_attention): 128 rows of a block must span less than 2 GiB -- true for every case here under both addressings,
    so none is diverted to the flash kernel"""
    for kernel, L, hd, dt, H, U, lay in CASES:
        for row_stride in (1, U):
            assert row_stride * 3 * H * hd * 2 * 128 < 2 ** 31


# ------------------------------------------------------------------------------------------------ GPU
@pytest.fixture
def kernel_choice(lib):
    """latte_debug_set_choice for the duration of a test (include/latte_amd_debug.h: another implementation of the same function)."""
    from latte_amd._lib import check
    used = []

    def choose(name, value):
        check(lib.latte_debug_set_choice(name.encode(), int(value)))
        used.append(name)
    yield choose
    for name in used:
        check(lib.latte_debug_set_choice(name.encode(), 0))


def _bits(t):
    return t.contiguous().view(torch.int16)


def _launch(lib, qkv, case, tag):
    """One launch into a NaN-prefilled out between sentinel guard rows -> [S, L, D] in sequence order"""
    from latte_amd._lib import check, ptr, stream_ptr
    kernel, L, hd, dt, H, U, lay = case
    S, D = B * U, H * hd
    rows = S * L
    row_of, sample_stride, seq_stride, row_stride = row_map(L, U, lay, qkv.device)
    assert sorted(row_of.flatten().tolist()) == list(range(rows))
    out = torch.full((rows + 2 * GUARD, D), float("nan"), device=qkv.device, dtype=qkv.dtype)
    out[:GUARD] = SENT
    out[GUARD + rows:] = SENT
    check(lib.latte_debug_attention(ptr(qkv), ptr(out[GUARD:]), S, L, H, hd, U, sample_stride, seq_stride, row_stride, DT[dt], stream_ptr()))
    torch.cuda.synchronize()
    sent = torch.full((GUARD, D), SENT, device=qkv.device, dtype=qkv.dtype)
    assert torch.equal(_bits(out[:GUARD]), _bits(sent)), f"{tag}: wrote in front of out"
    assert torch.equal(_bits(out[GUARD + rows:]), _bits(sent)), f"{tag}: wrote behind out"
    got = out[GUARD:GUARD + rows][row_of]
    bad = ~torch.isfinite(got).all(-1)
    assert not bool(bad.any()), (f"{tag}: {int(bad.sum())} rows not finite (unwritten, or NaN read from a guard); first (seq, token) "
                                 f"{tuple(int(i) for i in torch.nonzero(bad)[0])}")
    return got


@gpu
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_self_attention(lib, case, kernel_choice):
    kernel, L, hd, dt, H, U, lay = case
    dev = torch.device("cuda")
    variant = KERNELS[kernel][0]
    if variant:
        kernel_choice("attn_variant", variant)
    x = make_inputs(case, dev)
    want, bound = reference(x, kernel)
    row_of = row_map(L, U, lay, dev)[0]
    qkv = pack_rows(x, row_of)
    got = _launch(lib, qkv, case, _id(case))
    ratio = worst(_id(case), got, want, bound)
    again = _launch(lib, qkv, case, _id(case) + " (second launch)")
    assert torch.equal(_bits(again), _bits(got)), "the same launch twice gives different bits"
    x1 = x.clone()
    x1[U:] = make_inputs(case, dev, seed_shift=1)[U:]                     # sample 1's rows replaced
    other = _launch(lib, pack_rows(x1, row_of), case, _id(case) + " (sample 1 replaced)")
    assert torch.equal(_bits(other[:U]), _bits(got[:U])), "sample 0 changes with sample 1's rows"
    assert not torch.equal(_bits(other[U:]), _bits(got[U:]))
    print(f"self-attention {_id(case)}: worst err / bound {ratio:.3f}")
