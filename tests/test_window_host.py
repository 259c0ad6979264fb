"""The host side of sampling with overlapping temporal windows: the window set of ``latte_window_plan`` /
``latte_amd.window_starts`` over a grid of (L, F, stride), its refusals, and the NULL-handle refusals of every new entry point, which
come before any device is asked for.  No GPU."""
import ctypes

import pytest

import latte_amd
from latte_amd import LatteError

INVALID = 1
GRID = [(L, F, S) for F in (1, 2, 4, 16) for L in range(F, 3 * F + 3) for S in range(1, F + 1)]


def _plan(lib, L, F, S, cap=None):
    starts, counts = (ctypes.c_int * max(L, 1))(), (ctypes.c_int * max(L, 1))()
    W = lib.latte_window_plan(L, F, S, starts, counts, L if cap is None else cap)
    return W, list(starts)[:max(W, 0)], list(counts)[:L]


def test_window_plan_over_a_grid(lib):
    assert len(GRID) > 300
    for L, F, S in GRID:
        W, starts, counts = _plan(lib, L, F, S)
        assert W == -(-(L - F) // S) + 1, (L, F, S)
        assert starts == [min(w * S, L - F) for w in range(W)]
        assert starts[0] == 0 and starts[-1] == L - F and all(a < b for a, b in zip(starts, starts[1:]))
        assert min(counts) >= 1 and sum(counts) == W * F
        assert counts == [sum(s <= f < s + F for s in starts) for f in range(L)]
        assert latte_amd.window_starts(L, F, S) == starts and latte_amd.window_counts(L, F, S) == counts
    assert latte_amd.window_starts(10, 4, 3) == [0, 3, 6] and latte_amd.window_starts(9, 4, 3) == [0, 3, 5]
    assert latte_amd.window_starts(7, 4, 2) == [0, 2, 3] and latte_amd.window_starts(40, 16, 8) == [0, 8, 16, 24]
    assert latte_amd.window_starts(16, 16, 5) == [0]
    # either output may be left out
    assert lib.latte_window_plan(9, 4, 3, None, None, 0) == 3


def test_window_plan_refusals(lib):
    for (L, F, S), text in (((3, 4, 1), b"total_frames"), ((8, 4, 0), b"stride"), ((8, 4, -1), b"stride"), ((8, 4, 5), b"stride"),
                            ((8, 0, 1), b"total_frames")):
        W, _, _ = _plan(lib, L, F, S)
        assert W == -INVALID and b"window_plan" in lib.latte_last_error() and text in lib.latte_last_error(), (L, F, S)
        with pytest.raises(LatteError, match="window_plan"):
            latte_amd.window_starts(L, F, S)
    W, _, _ = _plan(lib, 9, 4, 3, cap=2)
    assert W == -INVALID and b"starts_out" in lib.latte_last_error()


def test_null_handles_are_refused_before_any_device_call(lib):
    assert lib.latte_window_gather(None, None, 1, 8, 4, 2, 4, 16, 0, None) == INVALID and b"window_gather" in lib.latte_last_error()
    assert lib.latte_window_merge(None, None, 1, 8, 4, 2, 8, 16, 0, None) == INVALID and b"window_merge" in lib.latte_last_error()
    assert lib.latte_sample_loop_windows(None, None, 1, 0.0, 1, 0, 1.0, None, None, 1, 1, 0, None, None, None, 8, 2, None) == INVALID
    assert b"sample_loop_windows" in lib.latte_last_error()
    assert lib.latte_sample_plan_loop_windows(None, 0, 1.0, None, None, 1, 1, None, None, None, 8, 2, None) == INVALID
    assert b"sample_plan_loop_windows" in lib.latte_last_error()
    assert lib.latte_t2v_guided_ddim_loop_windows(None, None, 1, 1, None, None, None, 4.0, 1, 8, 2, None) == INVALID
    assert b"t2v_guided_ddim_loop_windows" in lib.latte_last_error()
    assert lib.latte_t2v_guided_linear_loop_windows(None, None, 1, 1, None, None, 4.0, 1, 8, 2, None) == INVALID
    assert b"t2v_guided_linear_loop_windows" in lib.latte_last_error()


def test_host_refusals_of_the_public_loop():
    d = latte_amd.create_diffusion("10")

    class Model:
        num_frames = 4

        def __call__(self, x, t, **kw):
            return x

    for kw, text in ((dict(shape=(1, 3, 4, 8, 8)), "total_frames"), (dict(shape=(1, 8, 4, 8, 8), stride=5), "stride"),
                     (dict(shape=(1, 8, 4, 8, 8), stride=0), "stride"), (dict(shape=(1, 8, 4, 8, 8), method="plms"), "method"),
                     (dict(shape=(1, 8, 4, 3, 2)), "multiple of 4"), (dict(shape=(1, 8, 4, 8)), "shape must be")):
        with pytest.raises(LatteError, match=text):
            d.window_sample_loop(Model(), **kw)
    with pytest.raises(LatteError, match="num_frames"):
        d.window_sample_loop(lambda x, t: x, (1, 8, 4, 8, 8))
