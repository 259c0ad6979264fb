"""The patch embed's input gradient (csrc/train_fin.hip: patch_embed_dgrad_kernel, behind latte_trainer_input_grad) through its debug
hook: out [BF, C, G p, G p] = dx [BF G^2, D] W [D, C p^2] scattered to the pixels -- the inverse of im2col_patch.  Everything fp32.

Cases (D, C, p, G, BF): the fixture's width, a row count that is no multiple of a workgroup's eight rows, Latte-XL's width (4.5
16-byte chunks per lane), KPE = C p^2 = 64 (the last size of the one-wave-per-row form, 64 partial sums per lane) and KPE = 256 (the
plain product + scatter)."""
import pytest
import torch

CASES = [(128, 4, 2, 4, 3), (384, 4, 2, 3, 5), (1152, 4, 2, 4, 2), (128, 4, 4, 2, 3), (128, 4, 8, 2, 1),
         (128, 8, 2, 2, 1), (128, 3, 2, 2, 2)]     # the 32-sum instantiation; KPE = 12 inside the 16-sum one (an idle quarter of the sums)
IDS = ["D128", "D384-rows45", "D1152", "KPE64", "KPE256-wide", "KPE32", "KPE12"]


def reference(dx, W, BF, G, p, C):
    """fp64: dpix[m][(c, pp, q)] -> out[bf][c][gh p + pp][gw p + q], m = (bf G + gh) G + gw (x_embedder.proj.weight order)."""
    pix = dx.double() @ W.double()
    return pix.reshape(BF, G, G, C, p, p).permute(0, 3, 1, 4, 2, 5).reshape(BF, C, G * p, G * p)


def run(lib, dx, W, BF, G, p, C, D, scale=None):
    from latte_amd._lib import check, ptr, stream_ptr
    dev = torch.device("cuda")
    a, b = dx.to(dev).contiguous(), W.to(dev).contiguous()
    out = torch.full((BF, C, G * p, G * p), float("nan"), device=dev)
    s = None if scale is None else torch.tensor([scale], device=dev)
    check(lib.latte_debug_patch_embed_dgrad(ptr(a), ptr(b), ptr(out), BF, G, p, C, D, ptr(s) if s is not None else None, stream_ptr()))
    torch.cuda.synchronize()
    return out.cpu()


def inputs(D, C, p, G, BF):
    g = torch.Generator("cpu").manual_seed(D + 7 * p + G + BF)
    return torch.randn(BF * G * G, D, generator=g), torch.randn(D, C * p * p, generator=g) * 0.05


@pytest.mark.gpu
@pytest.mark.parametrize("D,C,p,G,BF", CASES, ids=IDS)
def test_against_fp64(lib, D, C, p, G, BF):
    """|err| <= D 2^-24 sum_d |dx[m][d]| |W[d][j]|: the bound of an fp32 sum of D terms in any order (products and partial sums each
    rounded once, to first order (D - 1 + 1) u of the summed magnitudes, u = 2^-24)."""
    dx, W = inputs(D, C, p, G, BF)
    got = run(lib, dx, W, BF, G, p, C, D).double()
    want = reference(dx, W, BF, G, p, C)
    bound = D * 2.0 ** -24 * reference(dx.abs(), W.abs(), BF, G, p, C)
    err = (got - want).abs()
    assert torch.isfinite(got).all()                       # every pixel written (the output started as NaN)
    print(f"D {D} KPE {C * p * p}: worst err / bound {float((err / bound).max()):.3g}")
    assert bool((err <= bound).all()), float((err / bound).max())


@pytest.mark.gpu
@pytest.mark.parametrize("D,C,p,G,BF", CASES, ids=IDS)
def test_layout_one_hot(lib, D, C, p, G, BF):
    """dx one-hot at (row m, column d): the output is W[d, :] in token m's patch, bit for bit, and zero everywhere else."""
    _, W = inputs(D, C, p, G, BF)
    M = BF * G * G
    for m, d in ((0, 0), (M - 1, D - 1), (M // 2 + 1, D // 2 + 3)):
        dx = torch.zeros(M, D)
        dx[m, d] = 1.0
        got = run(lib, dx, W, BF, G, p, C, D)
        want = torch.zeros(BF, C, G * p, G * p)
        bf, gh, gw = m // (G * G), (m // G) % G, m % G
        want[bf, :, gh * p:(gh + 1) * p, gw * p:(gw + 1) * p] = W[d].reshape(C, p, p)
        assert torch.equal(got, want), (m, d)


@pytest.mark.gpu
@pytest.mark.parametrize("D,C,p,G,BF", CASES, ids=IDS)
def test_loss_scale_leaves_exactly(lib, D, C, p, G, BF):
    """With the device loss scale 2^14 the result is the unscaled one times 2^-14 exactly (a power of two)."""
    dx, W = inputs(D, C, p, G, BF)
    plain = run(lib, dx, W, BF, G, p, C, D)
    scaled = run(lib, dx, W, BF, G, p, C, D, scale=2.0 ** 14)
    assert torch.equal(scaled, plain * 2.0 ** -14)
