"""Clips longer than ``video_length`` on the text-to-video chain: ``LattePipeline.__call__(video_length=L, window_stride=S)`` on the
tiny_t2v fixture (F = 4, 8 x 8 latents) and the pipe of tests/test_t2v_schedulers.py, L = 7 at stride 2 (windows at 0, 2, 3), one prompt:
2 x 3 = 6 clips per evaluation, ``max_batch`` 6.  The fused calls (``latte_t2v_guided_ddim_loop_windows``,
``latte_t2v_guided_linear_loop_windows``) against the Python loop with ``latte_window_gather`` / ``latte_window_merge`` at the 1e-5 that
file holds its fused chains to; against the fp32 oracle denoiser run per window and merged in torch at the project's 1e-3; L equal to
``video_length`` against the pipeline without windows, bit for bit; the refusals of the two entry points."""
import numpy as np
import pytest
import torch

import latte_amd
from latte_amd.schedulers import DDIMScheduler, DPMSolverMultistepScheduler
from _util import rel_l2
from test_t2v_schedulers import _fixture, _model

pytestmark = pytest.mark.gpu
STEPS, SCALE = 5, 4.5
L, STRIDE, STARTS = 7, 2, [0, 2, 3]
INVALID, STATE = 1, 3


@pytest.fixture(scope="module")
def t2v_pipe():
    cfg, sd = _fixture()
    pipe = latte_amd.LattePipeline(transformer=_model(cfg, sd, max_batch=6), scheduler=DDIMScheduler()).to("cuda")
    return cfg, sd, pipe


def _inputs(cfg, frames=L):
    g = torch.Generator("cpu").manual_seed(13)
    pe, ne = torch.randn(1, 6, cfg.caption_channels, generator=g), torch.randn(1, 6, cfg.caption_channels, generator=g)
    lat = torch.randn((1, 4, frames, cfg.sample_size, cfg.sample_size), generator=g)
    return pe, ne, lat


def _run(pipe, pe, ne, lat, fused, **kw):
    pipe.allow_fused_loop = fused
    try:
        return pipe(prompt_embeds=pe, negative_prompt_embeds=ne, num_inference_steps=STEPS, guidance_scale=SCALE, latents=lat,
                    video_length=lat.shape[2], output_type="latents", **kw).video
    finally:
        pipe.allow_fused_loop = True


def _oracle_loop(cfg, sd, sch, pe, ne, lat):
    """The guided loop with the fp32 oracle denoiser on every window of the pair, merged in torch (ascending windows, uniform mean)."""
    from oracle import latte_t2v_oracle as to
    F = cfg.video_length
    assert latte_amd.window_starts(L, F, STRIDE) == STARTS
    count = torch.tensor([sum(s <= f < s + F for s in STARTS) for f in range(L)], dtype=torch.float32)
    want = lat.clone() * sch.init_noise_sigma
    enc = torch.cat([ne, pe])
    with torch.no_grad():
        for t in sch.timesteps:
            x2 = sch.scale_model_input(torch.cat([want] * 2), t)
            acc = None
            for s in STARTS:
                out = to.latte_t2v_forward(sd, cfg, x2[:, :, s:s + F].contiguous(), t.reshape(1).expand(2), enc)
                pad = torch.zeros(out.shape[:2] + (L,) + out.shape[3:])
                pad[:, :, s:s + F] = out
                acc = pad if acc is None else acc + pad
            merged = acc / count[None, None, :, None, None]
            unc, txt = merged.chunk(2)
            eps = (unc + SCALE * (txt - unc)).chunk(2, dim=1)[0]
            want = sch.step(eps, t, want, return_dict=False)[0]
    return want


@pytest.mark.parametrize("cls", [DDIMScheduler, DPMSolverMultistepScheduler])
def test_fused_chain_matches_the_python_loop_and_the_oracle_loop(t2v_pipe, cls):
    cfg, sd, pipe = t2v_pipe
    pipe.scheduler = cls()
    pe, ne, lat = _inputs(cfg)
    tr = pipe.transformer
    lib = latte_amd.load_library()
    name = "guided_ddim_loop_windows" if cls is DDIMScheduler else "guided_linear_loop_windows"
    calls = {"fused": 0, "plain": 0, "gather": 0, "merge": 0}
    real = {k: getattr(lib, k) for k in ("latte_window_gather", "latte_window_merge")}

    def spy(*a, **kw):
        calls["fused"] += 1
        return getattr(type(tr), name)(tr, *a, **kw)

    def plain_spy(*a, **kw):
        calls["plain"] += 1
        raise AssertionError("the plain loop must not run on a windowed clip")

    def count(key, fn):
        def wrapper(*a):
            calls[key] += 1
            return fn(*a)
        return wrapper

    setattr(tr, name, spy)
    tr.guided_ddim_loop = tr.guided_linear_loop = plain_spy
    lib.latte_window_gather, lib.latte_window_merge = count("gather", real["latte_window_gather"]), count("merge", real["latte_window_merge"])
    try:
        fused = _run(pipe, pe, ne, lat, True, window_stride=STRIDE)
        assert calls == {"fused": 1, "plain": 0, "gather": 0, "merge": 0}, calls          # ONE engine call
        stepped = _run(pipe, pe, ne, lat, False, window_stride=STRIDE)
        assert calls == {"fused": 1, "plain": 0, "gather": STEPS, "merge": STEPS}, calls
    finally:
        delattr(tr, name)
        del tr.guided_ddim_loop, tr.guided_linear_loop
        lib.latte_window_gather, lib.latte_window_merge = real["latte_window_gather"], real["latte_window_merge"]
    assert fused.shape == lat.shape and torch.isfinite(fused).all()
    err = rel_l2(fused, stepped)
    print(f"{cls.__name__}: windowed chain, fused vs Python loop rel-L2 {err:.3e}")
    assert err < 1e-5
    sch = cls()
    sch.set_timesteps(STEPS)
    err = rel_l2(fused, _oracle_loop(cfg, sd, sch, pe, ne, lat))
    print(f"{cls.__name__}: windowed chain vs oracle loop rel-L2 {err:.3e}")
    assert err < 1e-3


@pytest.mark.parametrize("cls", [DDIMScheduler, DPMSolverMultistepScheduler])
@pytest.mark.parametrize("fused", [True, False])
def test_video_length_of_the_model_is_the_pipeline_without_windows(t2v_pipe, cls, fused):
    cfg, sd, pipe = t2v_pipe
    pipe.scheduler = cls()
    pe, ne, lat = _inputs(cfg, cfg.video_length)
    plain = _run(pipe, pe, ne, lat, fused)
    for stride in (1, 4):
        assert torch.equal(_run(pipe, pe, ne, lat, fused, window_stride=stride), plain)


def test_refusals(t2v_pipe):
    from latte_amd._lib import ptr, stream_ptr
    from latte_amd.schedulers import PLAN_COLS
    cfg, sd, pipe = t2v_pipe
    pipe.scheduler = DDIMScheduler()
    pe, ne, lat = _inputs(cfg)
    with pytest.raises(latte_amd.LatteError, match="window_plan"):
        _run(pipe, pe, ne, lat, True, window_stride=5)
    with pytest.raises(latte_amd.LatteError, match="window_plan"):
        _run(pipe, pe, ne, lat[:, :, :3], True, window_stride=2)
    with pytest.raises(latte_amd.LatteError, match="known-region"):
        _run(pipe, pe, ne, lat, True, window_stride=2, known_latents=lat, known_mask=torch.zeros(1, L, 8, 8))
    m, lib = pipe.transformer, latte_amd.load_library()
    assert m.max_batch == 6
    x = lat.cuda().contiguous()
    before = x.clone()
    ts = np.array([500, 0], dtype=np.int64)
    at, ap = np.array([0.3, 0.9]), np.array([0.9, 1.0])
    plan = np.zeros((2, PLAN_COLS))
    plan[:, 0], plan[:, 1], plan[:, 2], plan[:, 5] = [500, 0], 1.0, 1.0, 1.0

    def ddim(total=L, stride=STRIDE, samples=1):
        return lib.latte_t2v_guided_ddim_loop_windows(m._h, ptr(x), samples, 2, ts.ctypes.data, at.ctypes.data, ap.ctypes.data, SCALE, 1, total,
                                                      stride, stream_ptr())

    def linear(total=L, stride=STRIDE, samples=1):
        return lib.latte_t2v_guided_linear_loop_windows(m._h, ptr(x), samples, 2, plan.ctypes.data, None, SCALE, 1, total, stride, stream_ptr())

    for fn, who in ((ddim, b"t2v_guided_ddim_loop_windows"), (linear, b"t2v_guided_linear_loop_windows")):
        m.set_text(torch.cat([ne, pe]).repeat_interleave(3, dim=0))              # the 6 rows of the pair's clips
        for kw, code, text in ((dict(total=3), INVALID, b"total_frames"), (dict(stride=0), INVALID, b"stride"), (dict(stride=5), INVALID, b"stride"),
                               (dict(stride=1), STATE, b"max_batch"),              # 4 windows: 8 clips
                               (dict(samples=2), STATE, b"max_batch"),
                               (dict(total=6), STATE, b"text context")):           # 2 windows: 4 clips, 6 rows installed
            assert fn(**kw) == code and text in lib.latte_last_error() and who in lib.latte_last_error(), (kw, lib.latte_last_error())
        m.set_text(torch.cat([ne, pe]))                                          # the rows of the plain pair: mis-sized for 3 windows
        assert fn() == STATE and b"text context" in lib.latte_last_error()
        assert lib.latte_t2v_set_text(m._h, None, None, 0, 0, stream_ptr()) == 0   # none installed
        assert fn() == STATE and b"text context" in lib.latte_last_error()
    torch.cuda.synchronize()
    assert torch.equal(x, before)
