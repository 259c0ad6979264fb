"""What the trainer shows of its trained sets, for a plain trainer and a LoRA one (rank 4 on proj, fc1): the key sets of
``training_state()`` outside and inside an accumulation window, which public buffers are None, every flat buffer's size and every
``layout`` entry against the engine's accessors, the aliasing of the module's parameters, and ``load_training_state`` of the trainer's
own state as the identity on every flat buffer.  Fixture: oracle.make_golden.TRAIN_STEP at batch 2."""
import pytest
import torch

from oracle.make_golden import TRAIN_STEP, train_step_inputs

pytestmark = pytest.mark.gpu
BUFFERS = ("params", "grads", "exp_avg", "exp_avg_sq", "ema")
COUNTERS = {"scaler", "train_steps", "micro_step", "gradient_accumulation_steps"}


def make(lora):
    import latte_amd
    _, sd, x0, noise, t, y, drop = train_step_inputs()
    model = latte_amd.Latte(**TRAIN_STEP)
    model.load_state_dict(sd)
    kw = dict(lora_rank=4, lora_targets=("proj", "fc1")) if lora else {}
    tr = latte_amd.LatteTrainer(model.to("cuda"), latte_amd.create_diffusion(""), max_batch=2, lr=1e-3, gradient_accumulation_steps=2, **kw)
    return tr, [v[:2] for v in (x0, noise, t, y, drop)]


def engine_table(tr, family):
    from latte_amd._lib import load_library
    lib = load_library()
    fn = lambda name: getattr(lib, "latte_trainer_" + family + name)   # noqa: E731
    return ([(fn("param_key")(tr._h, i).decode(), int(fn("param_offset")(tr._h, i)), int(fn("param_numel")(tr._h, i)))
             for i in range(fn("num_params")(tr._h))], int(fn("total_numel")(tr._h)))


def flat_buffers(tr, lora):
    names = ["params"] + ["lora_" + b for b in BUFFERS] if lora else list(BUFFERS)
    return {n: getattr(tr, n) for n in names}


@pytest.mark.parametrize("lora", [False, True], ids=["plain", "lora"])
def test_state_keys_buffers_and_layout(lora):
    tr, (x0, noise, t, y, drop) = make(lora)
    # ---- which public buffers exist, their sizes and the layouts against the engine's accessors
    table, total = engine_table(tr, "")
    assert tr.layout == table and tr.params.numel() == total
    if lora:
        assert all(getattr(tr, b) is None for b in BUFFERS[1:])
        ltable, ltotal = engine_table(tr, "lora_")
        assert tr.lora_layout == ltable and len(ltable) == 2 * 2 * TRAIN_STEP["depth"]
        assert all(getattr(tr, "lora_" + b).numel() == ltotal for b in BUFFERS)
        assert [k for k, _, _ in ltable][:4] == ["blocks.0.attn.proj.lora_A", "blocks.0.attn.proj.lora_B",
                                                 "blocks.0.mlp.fc1.lora_A", "blocks.0.mlp.fc1.lora_B"]
    else:
        assert all(getattr(tr, b).numel() == total for b in BUFFERS)
        assert engine_table(tr, "lora_") == ([], 0)
    assert tr.check_aliasing()
    # ---- the key sets of the state: outside a window, then inside one of two
    trained_keys = {"config", "params", "ema", "exp_avg", "exp_avg_sq"}

    def check_keys(inside):
        st = tr.training_state()
        if lora:
            assert set(st) == {"model", "lora"} | COUNTERS
            assert set(st["lora"]) == trained_keys | ({"grads"} if inside else set())
            assert set(st["lora"]["exp_avg"]) == set(st["lora"]["params"]) == {k for k, _, _ in tr.lora_layout}
        else:
            assert set(st) == {"model", "ema", "opt"} | COUNTERS | ({"grads"} if inside else set())
            assert set(st["opt"]) == {"exp_avg", "exp_avg_sq"}
            assert set(st["opt"]["exp_avg"]) == {k for k, _, _ in tr.layout}
        assert set(st["model"]) == set(tr.model.state_dict())
        assert st["micro_step"] == int(inside)
        return st
    check_keys(False)
    for _ in range(2):                                                       # one whole window: moments and EMA leave zero / the parameters
        tr.train_step(x0, y=y, t=t, noise=noise, drop_mask=drop)
    out = tr.train_step(x0, y=y, t=t, noise=noise, drop_mask=drop)
    assert not out["updated"] and tr.micro_step == 1
    st = check_keys(True)
    # ---- load_training_state(training_state()) is the identity on every flat buffer
    before = {n: v.clone() for n, v in flat_buffers(tr, lora).items()}
    assert float(before["lora_grads" if lora else "grads"].abs().max()) > 0.0
    assert float(before["lora_exp_avg" if lora else "exp_avg"].abs().max()) > 0.0
    tr.load_training_state(st)
    torch.cuda.synchronize()
    for n, v in flat_buffers(tr, lora).items():
        assert torch.equal(v, before[n]), n
    assert tr.micro_step == 1 and tr.train_steps == 1 and tr.check_aliasing()
