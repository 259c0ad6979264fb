"""Known-region sampling, the parts that need no GPU: the slab count of ``latte_known_chain_slabs`` against a hand count, the mask
builder ``latte_amd.known_mask``, and the refusals that are decided on the host."""
import ctypes

import pytest
import torch

import known_reference as kr

INVALID = 1
DDPM, DDIM, DDIM_REVERSE = 0, 1, 2


def _slabs(lib, d, method, eta, start, end, resample, blend_start):
    n = ctypes.c_int64(-1)
    rc = lib.latte_known_chain_slabs(d._h, method, eta, start, end, resample, blend_start, ctypes.byref(n))
    return rc, n.value


@pytest.mark.parametrize("spec,T", [("50", 50), ("10", 10)])
def test_slab_count_against_a_hand_count(lib, spec, T):
    import latte_amd
    d = latte_amd.create_diffusion(spec)
    # written out for the full chain with the start blend: T - 1 indices above 0 take noise, index 0 takes none
    by_hand = {
        (DDPM, 0.0, 1): 1 + (T - 1) * 2,               # step + blend
        (DDIM, 0.0, 1): 1 + (T - 1) * 1,               # blend
        (DDIM, 0.5, 1): 1 + (T - 1) * 2,               # step + blend
        (DDPM, 0.0, 3): 1 + (T - 1) * (3 * 2 + 2),     # three repetitions and two jumps
        (DDIM, 0.0, 3): 1 + (T - 1) * (3 * 1 + 2),
        (DDIM, 0.5, 3): 1 + (T - 1) * (3 * 2 + 2),
    }
    for (method, eta, resample), want in by_hand.items():
        assert _slabs(lib, d, method, eta, T - 1, 0, resample, 1) == (0, want), (method, eta, resample)
        assert _slabs(lib, d, method, eta, T - 1, 0, resample, 0) == (0, want - 1)
        assert d.known_chain_slabs("ddpm" if method == DDPM else "ddim", eta, resample) == want
    # partial ranges, with and without the start blend, against the restatement's own count
    for method, name in ((DDPM, "ddpm"), (DDIM, "ddim")):
        for eta in (0.0, 1.0):
            for resample in (1, 3):
                for hi, lo in ((T - 1, 0), (T - 1, 5), (6, 0), (4, 4), (0, 0), (7, 1)):
                    for bs in (0, 1):
                        want = kr.slab_count(hi, lo, name, eta, resample, bs)
                        assert _slabs(lib, d, method, eta, hi, lo, resample, bs) == (0, want), (name, eta, resample, hi, lo, bs)
    # a chain split at k consumes what the single call consumes
    assert _slabs(lib, d, DDPM, 0.0, T - 1, 4, 3, 1)[1] + _slabs(lib, d, DDPM, 0.0, 3, 0, 3, 0)[1] == _slabs(lib, d, DDPM, 0.0, T - 1, 0, 3, 1)[1]
    # index 0 alone: no noise at all without the start blend
    assert _slabs(lib, d, DDPM, 0.0, 0, 0, 3, 0) == (0, 0)


def test_slab_count_refusals(lib):
    import latte_amd
    from latte_amd import LatteError
    d = latte_amd.create_diffusion("50")
    n = ctypes.c_int64(-1)
    assert _slabs(lib, d, DDPM, 0.0, 49, 0, 0, 1)[0] == INVALID and b"resample" in lib.latte_last_error()
    assert _slabs(lib, d, DDIM_REVERSE, 0.0, 49, 0, 1, 1)[0] == INVALID and b"method" in lib.latte_last_error()
    for hi, lo in ((50, 0), (3, 4), (5, -1)):
        assert _slabs(lib, d, DDIM, 0.0, hi, lo, 1, 1)[0] == INVALID and b"index range" in lib.latte_last_error()
    assert lib.latte_known_chain_slabs(None, DDIM, 0.0, 49, 0, 1, 1, ctypes.byref(n)) == INVALID
    assert lib.latte_known_chain_slabs(d._h, DDIM, 0.0, 49, 0, 1, 1, None) == INVALID
    with pytest.raises(LatteError, match="resample"):
        d.known_chain_slabs("ddim", resample=0)
    with pytest.raises(LatteError, match="method"):
        d.known_chain_slabs("euler")
    with pytest.raises(LatteError, match="index range"):
        d.known_chain_slabs("ddim", start_index=50)


def test_known_mask_shapes_and_values():
    import latte_amd
    from latte_amd import LatteError
    m = latte_amd.known_mask((2, 4, 8, 8), frames=[0, 3])
    assert m.shape == (2, 4, 8, 8) and m.dtype == torch.float32
    assert torch.equal(m, kr.mask_of((2, 4, 4, 8, 8), [0, 3]))
    assert float(m[:, [0, 3]].min()) == 1.0 and float(m[:, [1, 2]].max()) == 0.0
    m5 = latte_amd.known_mask((2, 4, 4, 8, 8), box=(2, 2, 6, 6))       # latents' shape: the channel axis is dropped
    assert m5.shape == (2, 4, 8, 8) and torch.equal(m5, kr.mask_of((2, 4, 4, 8, 8), None, (2, 2, 6, 6)))
    assert float(m5.sum()) == 2 * 4 * 16 and float(m5[:, :, 2:6, 2:6].min()) == 1.0
    both = latte_amd.known_mask((1, 3, 6, 4), frames=[-1], box=(0, 1, 2, 3))
    assert torch.equal(both, kr.mask_of((1, 3, 1, 6, 4), [2], (0, 1, 2, 3))) and float(both.sum()) == 24 + 2 * 4
    assert float(latte_amd.known_mask((1, 2, 4, 4)).sum()) == 0.0
    assert set(both.unique().tolist()) == {0.0, 1.0}
    for bad in (dict(shape=(2, 4, 8)), dict(shape=(2, 4, 8, 8), frames=[4]), dict(shape=(2, 4, 8, 8), frames=[-5]),
                dict(shape=(2, 4, 8, 8), box=(2, 2, 2, 6)), dict(shape=(2, 4, 8, 8), box=(0, 0, 9, 8)), dict(shape=(2, 4, 8, 8), box=(1, 2, 3)),
                dict(shape=(0, 4, 8, 8))):
        with pytest.raises(LatteError, match="known_mask"):
            latte_amd.known_mask(**bad)


def test_refusals_decided_on_the_host(lib):
    import latte_amd
    from latte_amd import LatteError
    d = latte_amd.create_diffusion("50")
    # the C entry points, before anything touches a device: NULL handles and operands
    assert lib.latte_sample_loop_known(None, d._h, DDIM, 0.0, 1, 0, 1.0, None, None, 2, 49, 0, None, None, 1, 1, None, None, None, None) == INVALID
    assert b"sample_loop_known" in lib.latte_last_error()
    assert lib.latte_known_blend(None, None, None, None, 0, 0, 1.0, 0.0, 1, 1, 1, 4, 0, None) == INVALID
    assert b"known_blend" in lib.latte_last_error()
    assert lib.latte_t2v_guided_ddim_loop_known(None, None, 1, 4, None, None, None, 7.5, None, None, None, 1, None) == INVALID
    assert b"t2v_guided_ddim_loop_known" in lib.latte_last_error()
    # the linear samplers have no known-region form
    x = torch.zeros(2, 4, 4, 8, 8)
    for kw in (dict(known=x), dict(known_mask=latte_amd.known_mask(x.shape, frames=[0])), dict(known=x, known_mask=latte_amd.known_mask(x.shape))):
        with pytest.raises(LatteError, match="linear samplers"):
            d.linear_sample_loop(lambda xx, t: xx, x.shape, **kw)
        with pytest.raises(LatteError, match="linear samplers"):
            next(d.linear_sample_loop_progressive(lambda xx, t: xx, x.shape, **kw))
    # known_sample_loop: the method, resample and the range are refused before a device is asked for
    mask = latte_amd.known_mask(x.shape, frames=[0])
    with pytest.raises(LatteError, match="method"):
        d.known_sample_loop(lambda xx, t: xx, x.shape, x, mask, method="heun", device="cpu")
    with pytest.raises(LatteError, match="resample"):
        d.known_sample_loop(lambda xx, t: xx, x.shape, x, mask, resample=0, device="cpu")
    with pytest.raises(LatteError, match="index range"):
        d.known_sample_loop(lambda xx, t: xx, x.shape, x, mask, start_index=3, end_index=4, device="cpu")
