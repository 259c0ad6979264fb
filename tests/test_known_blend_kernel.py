"""``known_blend_kernel`` (csrc/pointwise.hip) through ``latte_known_blend``, per element against the formula in fp64:

    x <- m == 1 ? kn : (m == 0 ? x : m kn + (1 - m) x),      kn = b == 0 ? known : a known + b z

in both latent layouts ([B, F, C, HW] and [B, C, F, HW]; the mask is [B, F, HW], shared by the channels), with mask values from
{0, 1, 0.25} per latent pixel plus one frame entirely 0 and one entirely 1 (whole 16-byte accesses that are skipped / replaced).

Bounds.  Where m == 0 the output is x bit for bit, where m == 1 and b == 0 it is ``known`` bit for bit: the kernel's two selects.  Where
m == 1 the output is a known + b z evaluated in fp32: two products and a sum, fused or not, each rounding at most 2^-24 relative of a
magnitude bounded by |a known| + |b z| -- bound 2^-22 (|a known| + |b z|).  For fractional m the same 2^-22 on the sum of the term
magnitudes m (|a known| + |b z|) + (1 - m) |x| (four more roundings of smaller terms; 2^-22 is four times 2^-24 of the sum, and every
partial result is below the sum).  The inline Philox draw is bit-identical to the explicit-noise launch fed from
``latte_debug_fill_normal`` at the same (seed, offset)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
INVALID = 1
SHAPES = [(3, 3, 4, 6), (1, 4, 4, 8), (2, 16, 4, 32)]   # (B, F, C, H = W): bpd_reference.K_SHAPES
EPS = 2.0 ** -22


def _inputs(shape, frames_inner, seed=0):
    B, F, C, H = shape
    g = torch.Generator("cpu").manual_seed(100 + seed + B * 10 + F)
    dims = (B, C, F, H, H) if frames_inner else (B, F, C, H, H)
    x, known, z = (torch.randn(dims, generator=g) for _ in range(3))
    mask = torch.tensor([0.0, 1.0, 0.25])[torch.randint(0, 3, (B, F, H, H), generator=g)]
    mask[0, 0] = 0.0              # whole accesses with nothing known
    mask[0, F - 1] = 1.0          # and with everything known
    return x, known, z, mask


def _blend(lib, x, known, mask, z, a, b, frames_inner, seed=0, offset=0):
    """One launch on a copy of x -> (rc, result)."""
    from latte_amd._lib import ptr, stream_ptr
    B, d1, d2, H, W = x.shape
    F, C = (d2, d1) if frames_inner else (d1, d2)
    xx = x.cuda().contiguous().clone()
    kn, mk = known.cuda().contiguous(), mask.cuda().contiguous()
    zz = None if z is None else z.cuda().contiguous()
    rc = lib.latte_known_blend(ptr(xx), ptr(kn), ptr(mk), ptr(zz), seed, offset, a, b, B, F, C, H * W, int(frames_inner), stream_ptr())
    torch.cuda.synchronize()
    return rc, xx.cpu()


def _m5(mask, frames_inner):
    return mask[:, None] if frames_inner else mask[:, :, None]      # broadcast over the channel axis of either layout


def _check(got, x, known, z, mask, a, b, frames_inner):
    a32, b32 = np.float32(a), np.float32(b)
    m = _m5(mask, frames_inner).expand_as(x)
    x64, k64, m64 = x.double(), known.double(), m.double()
    if b32 == 0:
        kn64, mag = k64, k64.abs()
    else:
        kn64 = float(a32) * k64 + float(b32) * z.double()
        mag = (float(a32) * k64).abs() + (float(b32) * z.double()).abs()
    zero, one, frac = m == 0, m == 1, (m != 0) & (m != 1)
    assert zero.any() and one.any() and frac.any()
    assert torch.equal(got[zero], x[zero])                                               # bit for bit
    if b32 == 0:
        assert torch.equal(got[one], known[one])                                         # known exactly
    d = (got.double() - kn64).abs()
    assert bool((d[one] <= EPS * mag[one]).all()), float((d[one] / mag[one]).max())
    want = m64 * kn64 + (1 - m64) * x64
    terms = m64 * mag + (1 - m64) * x64.abs()
    d = (got.double() - want).abs()
    worst = float((d[frac] / terms[frac]).max())
    print(tuple(x.shape), "layout", int(frames_inner), "a, b", a, b, "worst fractional error / term sum", worst, "of", EPS)
    assert bool((d[frac] <= EPS * terms[frac]).all()), worst


@pytest.mark.parametrize("frames_inner", [False, True], ids=["BFCHW", "BCFHW"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_per_element_against_the_formula(lib, shape, frames_inner):
    x, known, z, mask = _inputs(shape, frames_inner)
    for a, b in ((0.8, 0.6), (float(np.sqrt(np.float32(0.9999))), float(np.sqrt(np.float32(1) - np.float32(0.9999)))), (1.0, 0.0)):
        rc, got = _blend(lib, x, known, mask, z if b else None, a, b, frames_inner)
        assert rc == 0, lib.latte_last_error()
        _check(got, x, known, z, mask, a, b, frames_inner)
    # b == 0 never reads the noise: a slab of NaN changes nothing
    rc, got_nan = _blend(lib, x, known, mask, torch.full_like(z, float("nan")), 1.0, 0.0, frames_inner)
    assert rc == 0 and torch.equal(got_nan, got)
    # the two layouts are the same blend on permuted data
    if not frames_inner:
        p = lambda t: t.permute(0, 2, 1, 3, 4).contiguous()
        rc, a_ = _blend(lib, x, known, mask, z, 0.8, 0.6, False)
        rc2, b_ = _blend(lib, p(x), p(known), mask, p(z), 0.8, 0.6, True)
        assert rc == 0 and rc2 == 0 and torch.equal(p(a_), b_)


def test_non_finite_values_stay_where_the_mask_puts_them(lib):
    """The selects: an infinity in the unknown part of ``known`` / ``z`` never reaches x, and one in the replaced part of x never survives."""
    x, known, z, mask = _inputs(SHAPES[1], False)
    m = _m5(mask, False).expand_as(x)
    known, z, x = known.clone(), z.clone(), x.clone()
    known[m == 0] = float("inf")
    z[m == 0] = float("nan")
    x[m == 1] = float("inf")
    rc, got = _blend(lib, x, known, mask, z, 0.8, 0.6, False)
    assert rc == 0 and bool(torch.isfinite(got).all())
    assert torch.equal(got[m == 0], x[m == 0])


@pytest.mark.parametrize("frames_inner", [False, True], ids=["BFCHW", "BCFHW"])
@pytest.mark.parametrize("offset", [0, 4 * 1000, 4 * 123457 + 3, (1 << 33) + 8], ids=["0", "4k", "unaligned", "above_2_33"])
def test_inline_draw_is_the_generator_bit_for_bit(lib, offset, frames_inner):
    from latte_amd._lib import check, ptr, stream_ptr
    shape = SHAPES[2] if offset == 0 else SHAPES[0]
    x, known, _, mask = _inputs(shape, frames_inner, seed=1)
    seed = 0x1234567890ABCDEF
    z = torch.empty(x.shape, device="cuda", dtype=torch.float32)
    check(lib.latte_debug_fill_normal(ptr(z), z.numel(), seed, offset, stream_ptr()))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(z).all()) and 0.9 < float(z.std()) < 1.1
    rc1, explicit = _blend(lib, x, known, mask, z.cpu(), 0.8, 0.6, frames_inner)
    rc2, inline = _blend(lib, x, known, mask, None, 0.8, 0.6, frames_inner, seed, offset)
    assert rc1 == 0 and rc2 == 0
    assert torch.equal(explicit, inline)
    rc3, other = _blend(lib, x, known, mask, None, 0.8, 0.6, frames_inner, seed, offset + 4)      # and it does depend on the offset
    assert rc3 == 0 and not torch.equal(other, inline)


def test_refusals_leave_x_untouched(lib):
    x, known, z, mask = (torch.randn(1, 2, 4, 5, 5), torch.randn(1, 2, 4, 5, 5), torch.randn(1, 2, 4, 5, 5), torch.ones(1, 2, 5, 5))
    rc, got = _blend(lib, x, known, mask, z, 0.8, 0.6, False)           # H * W = 25
    assert rc == INVALID and b"multiple of 4" in lib.latte_last_error() and torch.equal(got, x)
    from latte_amd._lib import ptr, stream_ptr
    xx = torch.randn(1, 2, 4, 4, 4, device="cuda")
    before = xx.clone()
    for kn, mk in ((None, xx), (xx, None)):
        assert lib.latte_known_blend(ptr(xx), ptr(kn), ptr(mk), None, 0, 0, 0.8, 0.6, 1, 2, 4, 16, 0, stream_ptr()) == INVALID
        assert b"null" in lib.latte_last_error()
    assert lib.latte_known_blend(ptr(xx), ptr(xx), ptr(xx), None, 0, 0, 0.8, 0.6, 0, 2, 4, 16, 0, stream_ptr()) == INVALID
    torch.cuda.synchronize()
    assert torch.equal(xx, before)


def test_python_wrapper(lib):
    import latte_amd
    from latte_amd.known import level_coefs
    x, known, z, mask = _inputs(SHAPES[1], False)
    a, b = level_coefs(0.37)
    assert a == float(np.sqrt(np.float32(0.37))) and b == float(np.sqrt(np.float32(1) - np.float32(0.37)))
    rc, want = _blend(lib, x, known, mask, z, a, b, False)
    xx = x.cuda()
    out = latte_amd.known_blend(xx, known, mask, a, b, z)
    assert out is xx and torch.equal(out.cpu(), want)
    with pytest.raises(latte_amd.LatteError, match="mask"):
        latte_amd.known_blend(xx, known, mask[:, :2], a, b, z)
