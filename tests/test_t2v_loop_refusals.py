"""The argument block the three guided text-to-video loops share -- ``latte_t2v_guided_ddim_loop``, ``latte_t2v_guided_ddim_loop_known``
and ``latte_t2v_guided_linear_loop`` -- on the tiny_t2v fixture (max_batch 4): every refusal carries the entry point's own prefix and
comes before the first launch, so the latents keep their bits."""
import numpy as np
import pytest
import torch

from test_t2v_schedulers import _fixture, _model

pytestmark = pytest.mark.gpu
INVALID, STATE = 1, 3
SCALE = 4.5
LOOPS = ["t2v_guided_ddim_loop", "t2v_guided_ddim_loop_known", "t2v_guided_linear_loop"]


@pytest.fixture(scope="module")
def t2v():
    cfg, sd = _fixture()
    return cfg, _model(cfg, sd, max_batch=4).to("cuda")


def _latents(cfg, samples, seed=3):
    g = torch.Generator("cpu").manual_seed(seed)
    return torch.randn(max(samples, 1), 4, cfg.video_length, cfg.sample_size, cfg.sample_size, generator=g).cuda()


def _call(lib, m, loop, x, samples, n, alpha_t=None):
    """One raw call of `loop` with `n` steps (rows) on `x`; every other argument is a good one -> return code."""
    from latte_amd._lib import ptr, stream_ptr
    if loop == "t2v_guided_linear_loop":
        plan = np.zeros((n, 12), dtype=np.float64)                        # the step cap is checked before any row is read
        return lib.latte_t2v_guided_linear_loop(m._h, ptr(x), samples, n, plan.ctypes.data, None, SCALE, 1, stream_ptr())
    ts = np.ascontiguousarray(np.linspace(900, 0, n).astype(np.int64))
    at = np.full(n, 0.5) if alpha_t is None else np.asarray(alpha_t, dtype=np.float64)
    ap = np.full(n, 0.75)
    head = (m._h, ptr(x), samples, n, ts.ctypes.data, at.ctypes.data, ap.ctypes.data, SCALE)
    if loop == "t2v_guided_ddim_loop":
        return lib.latte_t2v_guided_ddim_loop(*head, 1, stream_ptr())
    kn, mk = torch.zeros_like(x), torch.zeros(x.shape[0], *x.shape[2:], device="cuda")
    nz = torch.zeros(n, *x.shape, device="cuda")
    return lib.latte_t2v_guided_ddim_loop_known(*head, ptr(kn), ptr(mk), ptr(nz), 1, stream_ptr())


@pytest.mark.parametrize("loop", LOOPS)
def test_shared_argument_block(lib, t2v, loop):
    from latte_amd._lib import check, stream_ptr
    cfg, m = t2v
    emb = torch.randn(4, 6, cfg.caption_channels, generator=torch.Generator("cpu").manual_seed(1))
    prefix = loop.encode() + b": "

    def refused(samples, n, code, text, rows=None):
        if rows is None:
            check(lib.latte_t2v_set_text(m._h, None, None, 0, 0, stream_ptr()))       # uninstalled
        else:
            m.set_text(emb[:rows])
        x = _latents(cfg, samples)
        keep = x.clone()
        rc = _call(lib, m, loop, x, samples, n)
        err = lib.latte_last_error()
        torch.cuda.synchronize()
        assert rc == code and err.startswith(prefix) and text in err, (rc, err)
        assert torch.equal(x, keep)

    m.set_text(emb[:2])                                                             # the engine exists from here on
    refused(0, 3, INVALID, b"bad arguments", rows=2)                                # samples = 0
    refused(3, 3, STATE, b"max_batch", rows=2)                                      # 2 * samples = 6 > max_batch = 4
    refused(1, 3, STATE, b"text context")                                           # no text context
    refused(1, 3, STATE, b"text context", rows=1)                                   # one row installed, the pair needs two
    refused(2, 3, STATE, b"text context", rows=2)                                   # the context of another batch
    refused(1, 1025, INVALID, b"more than 1024", rows=2)                            # more steps than the cap


def test_plain_ddim_loop_refuses_a_bad_alpha_table_up_front(lib, t2v):
    cfg, m = t2v
    m.set_text(torch.randn(2, 6, cfg.caption_channels, generator=torch.Generator("cpu").manual_seed(1)))
    x = _latents(cfg, 1)
    keep = x.clone()
    rc = _call(lib, m, "t2v_guided_ddim_loop", x, 1, 3, alpha_t=[0.5, 1.5, 0.5])
    err = lib.latte_last_error()
    torch.cuda.synchronize()
    assert rc == INVALID and err.startswith(b"t2v_guided_ddim_loop: ") and b"alpha out of range" in err, (rc, err)
    assert torch.equal(x, keep)                                                     # refused before step 0, not after it
