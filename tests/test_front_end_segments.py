"""The segment walk of the Python front end on the engine path: ``p_sample_loop_progressive``, ``ddim_sample_loop_progressive``
(eta 0.5) and ``ddim_reverse_sample_loop_progressive`` with ``SEGMENT_BYTES`` cut to three indices per engine call yield, bit for
bit, what the single-call run yields -- every trail entry and the final sample -- and the non-progressive method returns the last
progressive sample.  The torch draws are one ``randn_like`` per step in step order whatever the split, so a reseeded run repeats them.
tiny_classcond / tiny_uncond golden models, f16 operands, ``create_diffusion("10")``."""
import pytest
import torch

from _util import engine_model, load_golden_model

pytestmark = pytest.mark.gpu
SEED = 31
_CACHE = {}
LOOPS = {  # name -> (progressive method, its non-progressive form, the engine call, extra kwargs)
    "p_sample": ("p_sample_loop_progressive", "p_sample_loop", "latte_sample_loop_ex", {}),
    "ddim_eta0.5": ("ddim_sample_loop_progressive", "ddim_sample_loop", "latte_sample_loop_ex", {"eta": 0.5}),
    "ddim_reverse": ("ddim_reverse_sample_loop_progressive", "ddim_reverse_sample_loop", "latte_invert_loop", {}),
}


def _case(name, B, guided):
    """-> (model callable, start latents [B, ...] on the GPU, model_kwargs)"""
    if name not in _CACHE:
        kw, sd, _ = load_golden_model(name)
        _CACHE[name] = (kw, engine_model(kw, sd, "f16", max_batch=4))
    kw, m = _CACHE[name]
    g = torch.Generator("cpu").manual_seed(5)
    half = B // 2 if guided else B
    x = torch.randn(half, kw["num_frames"], 4, kw["input_size"], kw["input_size"], generator=g)
    mk = {}
    if kw["extras"] == 2:
        y = torch.randint(0, kw["num_classes"], (half,), generator=g)
        mk["y"] = (torch.cat([y, torch.full_like(y, kw["num_classes"])]) if guided else y).cuda()
    if guided:
        x, mk["cfg_scale"] = torch.cat([x, x]), 4.0
    return (m.forward_with_cfg if guided else m.forward), x.cuda().contiguous(), mk


def _run(d, method, fn, x, mk, extra):
    torch.manual_seed(SEED)
    args = (fn, x) if "reverse" in method else (fn, x.shape, x)
    out = getattr(d, method)(*args, model_kwargs=mk, **extra)
    return out if torch.is_tensor(out) else [(r["sample"].clone(), r["pred_xstart"].clone()) for r in out]


@pytest.mark.parametrize("model,B,guided", [("tiny_classcond", 2, False), ("tiny_classcond", 4, True), ("tiny_uncond", 2, False)])
@pytest.mark.parametrize("loop", list(LOOPS))
def test_segmented_run_is_the_single_segment_run(monkeypatch, lib, loop, model, B, guided):
    import latte_amd
    progressive, plain, entry, extra = LOOPS[loop]
    d = latte_amd.create_diffusion("10")
    fn, x, mk = _case(model, B, guided)
    calls = [0]
    real = getattr(lib, entry)

    def counted(*a):
        calls[0] += 1
        return real(*a)
    monkeypatch.setattr(lib, entry, counted, raising=False)
    x_before = x.clone()
    whole = _run(d, progressive, fn, x, mk, extra)
    assert calls[0] == 1 and len(whole) == 10
    monkeypatch.setattr(type(d), "SEGMENT_BYTES", 3 * x.numel() * 4)
    calls[0] = 0
    split = _run(d, progressive, fn, x, mk, extra)
    assert calls[0] == 4 and len(split) == 10                                         # 3 + 3 + 3 + 1 indices
    for k in range(10):
        assert torch.equal(split[k][0], whole[k][0]) and torch.equal(split[k][1], whole[k][1]), k
    assert all(torch.isfinite(s).all() for s, _ in whole) and not torch.equal(whole[0][0], whole[-1][0])
    calls[0] = 0
    final = _run(d, plain, fn, x, mk, extra)
    # the inversion splits only for its trails; the sampling loops split their noise as well
    assert calls[0] == (1 if loop == "ddim_reverse" else 4)
    assert torch.equal(final, whole[-1][0]) and torch.equal(x, x_before)             # the input is not written
    monkeypatch.undo()
    final = _run(d, plain, fn, x, mk, extra)                                          # one segment
    assert torch.equal(final, whole[-1][0])
