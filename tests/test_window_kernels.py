"""``window_gather_kernel`` and ``window_merge_kernel`` (csrc/pointwise.hip) through ``latte_window_gather`` / ``latte_window_merge``, in
both layouts: the gather against the torch slices bit for bit; the merge against the fp32 torch sum in the same (ascending window)
order -- bit for bit where one window covers a frame, within 1e-6 relative elsewhere (at most F fp32 additions in the same order and
one division, whose rounding may differ from torch's by an ulp: 2^-23 = 1.2e-7 per operation).  NaN-filled guards on both sides of every
output show that nothing outside it is written.

Shapes: G = 3, Cout = 8, HW = 4 (one 16-byte access per row) and 64; (L, F, stride) = (9, 4, 3) irregular tail, (4, 4, 2) one window,
(8, 4, 4) no overlap, (7, 4, 1) every interior frame covered four times."""
import pytest
import torch

import latte_amd

pytestmark = pytest.mark.gpu
INVALID = 1
G, C = 3, 8
SHAPES = [(9, 4, 3), (4, 4, 2), (8, 4, 4), (7, 4, 1)]
GUARD = 64


def _guarded(numel):
    buf = torch.full((numel + 2 * GUARD,), float("nan"), device="cuda")
    return buf, buf[GUARD:GUARD + numel]


def _guards_intact(buf):
    return bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all())


def _long(L, hw, inner, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((G, C, L, hw) if inner else (G, L, C, hw), generator=g).cuda()


def _slices(x, F, starts, inner):
    return torch.stack([x[g, :, s:s + F] if inner else x[g, s:s + F] for g in range(x.shape[0]) for s in starts])


@pytest.mark.parametrize("inner", [0, 1])
@pytest.mark.parametrize("hw", [4, 64])
@pytest.mark.parametrize("L,F,S", SHAPES)
def test_gather_is_the_torch_slices(lib, L, F, S, hw, inner):
    from latte_amd._lib import ptr, stream_ptr
    starts = latte_amd.window_starts(L, F, S)
    W = len(starts)
    x = _long(L, hw, inner, 1)
    want = _slices(x, F, starts, inner).contiguous()
    buf, out = _guarded(want.numel())
    assert lib.latte_window_gather(ptr(x), ptr(out), G, L, F, S, C, hw, inner, stream_ptr()) == 0, lib.latte_last_error()
    torch.cuda.synchronize()
    assert torch.equal(out.view(want.shape), want) and _guards_intact(buf)
    assert want.shape[0] == G * W
    # the Python wrapper, on [.., H, W] tensors
    h = 2 if hw == 4 else 8
    clips = latte_amd.window_gather(x.view(*x.shape[:3], h, hw // h), F, S, frames_inner=bool(inner))
    assert torch.equal(clips.flatten(3), want)


@pytest.mark.parametrize("inner", [0, 1])
@pytest.mark.parametrize("hw", [4, 64])
@pytest.mark.parametrize("L,F,S", SHAPES)
def test_merge_is_the_ordered_fp32_mean(lib, L, F, S, hw, inner):
    from latte_amd._lib import ptr, stream_ptr
    starts = latte_amd.window_starts(L, F, S)
    counts = latte_amd.window_counts(L, F, S)
    W = len(starts)
    g = torch.Generator().manual_seed(2)
    out = torch.randn((G * W, C, F, hw) if inner else (G * W, F, C, hw), generator=g).cuda()
    fr = (lambda t, f: t[:, f]) if inner else (lambda t, f: t[f])       # frame f of one clip / one merged row
    want = torch.empty((G, C, L, hw) if inner else (G, L, C, hw), device="cuda")
    for gi in range(G):
        for f in range(L):
            acc, n = None, 0
            for w, s in enumerate(starts):
                if s <= f < s + F:
                    v = fr(out[gi * W + w], f - s)
                    acc = v if acc is None else acc + v
                    n += 1
            assert n == counts[f]
            fr(want[gi], f).copy_(acc if n == 1 else acc / n)
    buf, merged = _guarded(want.numel())
    assert lib.latte_window_merge(ptr(out), ptr(merged), G, L, F, S, C, hw, inner, stream_ptr()) == 0, lib.latte_last_error()
    torch.cuda.synchronize()
    merged = merged.view(want.shape)
    assert _guards_intact(buf) and bool(torch.isfinite(merged).all())
    once = torch.tensor([c == 1 for c in counts], device="cuda")
    sel = (lambda t, m: t[:, :, m]) if inner else (lambda t, m: t[:, m])
    assert torch.equal(sel(merged, once), sel(want, once))
    if (~once).any():
        a, b = sel(merged, ~once), sel(want, ~once)
        err = float(((a - b).abs() / b.abs().clamp_min(1e-30)).max())
        print(f"merge (L, F, stride) = {(L, F, S)}, hw {hw}, frames_inner {inner}: worst relative error {err:.2e}")
        assert err <= 1e-6, err
    h = 2 if hw == 4 else 8
    got = latte_amd.window_merge(out.view(*out.shape[:3], h, hw // h), L, S, frames_inner=bool(inner))
    assert torch.equal(got.flatten(3), merged)


def test_gather_then_merge_returns_the_clip(lib):
    """The mean of equal values is the value where the sum of n copies and its division by n are exact (n <= 2), and within an ulp or
    two of it elsewhere."""
    L, F, S = 7, 4, 1
    x = _long(L, 64, 0, 3).view(G, L, C, 8, 8)
    assert set(latte_amd.window_counts(L, F, S)) == {1, 2, 3, 4}
    back = latte_amd.window_merge(latte_amd.window_gather(x, F, S), L, S)
    exact = torch.tensor([c <= 2 for c in latte_amd.window_counts(L, F, S)], device="cuda")
    assert torch.equal(back[:, exact], x[:, exact])
    assert float((back - x).abs().max()) <= 2e-7 * float(x.abs().max())


def test_refusals(lib):
    from latte_amd._lib import ptr, stream_ptr
    x = torch.zeros(G * 9 * C * 8, device="cuda")
    buf, out = _guarded(G * 3 * 4 * C * 8)
    for fn in (lib.latte_window_gather, lib.latte_window_merge):
        for args, text in (((G, 9, 4, 3, C, 6), b"multiple of 4"), ((G, 3, 4, 1, C, 8), b"total_frames"), ((G, 9, 4, 0, C, 8), b"stride"),
                           ((G, 9, 4, 5, C, 8), b"stride"), ((0, 9, 4, 3, C, 8), b"bad shape"), ((G, 9, 4, 3, 0, 8), b"bad shape")):
            assert fn(ptr(x), ptr(out), *args, 0, stream_ptr()) == INVALID and text in lib.latte_last_error(), (args, lib.latte_last_error())
        assert fn(None, ptr(out), G, 9, 4, 3, C, 8, 0, stream_ptr()) == INVALID and fn(ptr(x), None, G, 9, 4, 3, C, 8, 0, stream_ptr()) == INVALID
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all())
    with pytest.raises(latte_amd.LatteError, match="multiple of 4"):
        latte_amd.window_gather(torch.zeros(1, 8, 4, 3, 2, device="cuda"), 4, 2)
    with pytest.raises(latte_amd.LatteError, match="multiple"):
        latte_amd.window_merge(torch.zeros(5, 4, 8, 2, 2, device="cuda"), 8, 2)
