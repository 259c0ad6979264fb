"""Exact resume of a training run (LatteTrainer.training_state / load_training_state, latte_trainer_set_scaler_state): a run
interrupted after any micro-batch and continued on a fresh trainer over a fresh model ends with the same bits as the run that was
never interrupted -- parameters, EMA, both AdamW moments and all eight loss-scale / update counters."""
import functools
import io

import pytest
import torch

from oracle import latte_oracle as lo
from oracle.make_golden import TRAIN_STEP, train_step_inputs

A = 2                  # micro-batches per optimiser step
STEPS = 4              # optimiser steps of a history


@functools.lru_cache(maxsize=None)
def inputs():
    """Fixed (x_start, t, noise, y, drop) of every micro-batch of the history: batches of 2, labels repeat and drop."""
    g = torch.Generator("cpu").manual_seed(97)
    out = []
    for _ in range(A * STEPS):
        x0 = (torch.randn(2, 4, 4, 8, 8, generator=g) * 0.6).clamp(-1.0, 1.0)
        out.append((x0, torch.randint(0, 1000, (2,), generator=g), torch.randn(2, 4, 4, 8, 8, generator=g),
                    torch.randint(0, TRAIN_STEP["num_classes"], (2,), generator=g), torch.rand(2, generator=g) < 0.3))
    return out


def trainer(seed, custom_scale):
    import latte_amd
    model = latte_amd.Latte(**TRAIN_STEP)
    model.load_state_dict(train_step_inputs()[1] if seed is None else lo.init_state_dict(lo.LatteConfig(**TRAIN_STEP), seed=seed))
    # clipping starts inside the history (train_steps must come back), lr large enough that every step moves every parameter
    tr = latte_amd.LatteTrainer(model.to("cuda"), latte_amd.create_diffusion(""), max_batch=2, lr=1e-3, start_clip_iter=3,
                                gradient_accumulation_steps=A)
    if custom_scale:
        # a scale and a growth count that are not the defaults: the scale doubles after 3 applied updates -- inside the second half
        # of the history, and only there if `good_steps` (2 at the save) came back
        tr.set_option("loss_scale", 2 ** 12)
        tr.set_option("loss_scale_growth_interval", 3)
    return tr


def run(tr, first, last):
    for n in range(first, last):
        x0, t, noise, y, drop = inputs()[n]
        tr.train_step(x0, y=y, t=t, noise=noise, drop_mask=drop)
    torch.cuda.synchronize()


def snapshot(tr):
    return {"params": tr.params.clone(), "ema": tr.ema.clone(), "exp_avg": tr.exp_avg.clone(), "exp_avg_sq": tr.exp_avg_sq.clone(),
            "scaler": tr.scaler_state(), "train_steps": tr.train_steps, "micro_step": tr.micro_step}


@functools.lru_cache(maxsize=None)
def uninterrupted(custom_scale):
    tr = trainer(None, custom_scale)
    run(tr, 0, A * STEPS)
    return snapshot(tr)


@pytest.mark.gpu
@pytest.mark.parametrize("variant,cut", [("step boundary", 2 * A), ("mid-window", 2 * A + 1), ("custom scale", 2 * A)])
def test_resumed_run_is_bit_identical(variant, cut):
    custom = variant == "custom scale"
    want = uninterrupted(custom)
    first = trainer(None, custom)
    run(first, 0, cut)
    state = first.training_state()
    assert state["micro_step"] == cut % A and state["train_steps"] == cut // A and ("grads" in state) == bool(cut % A)
    assert set(state) >= {"model", "ema", "opt", "scaler", "train_steps", "micro_step"} and set(state["opt"]) == {"exp_avg", "exp_avg_sq"}
    assert set(state["opt"]["exp_avg"]) == {k for k, _, _ in first.layout} and len(state["scaler"]) == 8
    if custom:
        assert state["scaler"]["loss_scale"] == 2.0 ** 12 and state["scaler"]["good_steps"] == 2.0
    buf = io.BytesIO()
    torch.save(state, buf)
    del first, state
    buf.seek(0)
    state = torch.load(buf, map_location="cpu")
    second = trainer(12, False)                       # other weights, default scale and policy: all of it must come from the state
    second.load_training_state(state)
    assert second.check_aliasing()
    run(second, cut, A * STEPS)
    got = snapshot(second)
    for k in ("params", "ema", "exp_avg", "exp_avg_sq"):
        assert torch.equal(got[k], want[k]), k
    assert got["scaler"] == want["scaler"], (got["scaler"], want["scaler"])
    assert got["train_steps"] == want["train_steps"] == STEPS and got["micro_step"] == 0
    if custom:
        assert want["scaler"]["loss_scale"] == 2.0 ** 13 and want["scaler"]["applied_updates"] == 4.0


@pytest.mark.gpu
def test_model_and_ema_alone_do_not_resume_the_run():
    """What `pretrained:` restores -- the behaviour the feature replaces: fresh moments, bias correction from step 1."""
    want = uninterrupted(False)
    first = trainer(None, False)
    run(first, 0, 2 * A)
    sd, ema = first.model_state_dict(), first.ema_state_dict()
    second = trainer(12, False)
    second.load_state_dict(sd, ema)
    second.train_steps = 2
    run(second, 2 * A, A * STEPS)
    assert not torch.equal(second.params, want["params"])
    assert not torch.equal(second.exp_avg, want["exp_avg"])
    assert second.scaler_state()["applied_updates"] == 2.0 and want["scaler"]["applied_updates"] == 4.0


@pytest.mark.gpu
def test_set_scaler_state_validates():
    import latte_amd
    tr = trainer(None, False)
    st = tr.scaler_state()
    tr.set_scaler_state(dict(st, loss_scale=2.0 ** 10, good_steps=7.0, applied_updates=123.0, skipped_updates=2.0))
    back = tr.scaler_state()
    assert back["loss_scale"] == 2.0 ** 10 and back["good_steps"] == 7.0 and back["applied_updates"] == 123.0 and back["skipped_updates"] == 2.0
    with pytest.raises(latte_amd.LatteError):
        tr.set_scaler_state(dict(st, loss_scale=1000.0))
    with pytest.raises(latte_amd.LatteError):
        tr.set_scaler_state(dict(st, applied_updates=-1.0))
