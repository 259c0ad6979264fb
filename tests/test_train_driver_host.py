"""Host side of the training driver (tools/train.py, latte_amd/train_util.py): checkpoint format, learning-rate schedule, which
checkpoint a resumed run picks, and the data index of a micro-batch.  No GPU."""
import os

import pytest
import torch

from latte_amd import train_util as tu


def test_checkpoint_with_run_state_keys_is_read_by_find_model(tmp_path):
    """find_model (utils.py:274-287) takes the "ema" entry whatever else the file holds."""
    import latte_amd
    ck = {"model": {"w": torch.zeros(3)}, "ema": {"w": torch.ones(3)},
          "opt": {"exp_avg": {"w": torch.zeros(3)}, "exp_avg_sq": {"w": torch.zeros(3)}},
          "scaler": {"loss_scale": 16384.0, "applied_updates": 10.0}, "train_steps": 10, "rng": tu.rng_state()}
    path = str(tmp_path / "0000010.pt")
    torch.save(ck, path)
    sd = latte_amd.find_model(path)
    assert set(sd) == {"w"} and torch.equal(sd["w"], torch.ones(3))


def test_warmup_schedule():
    lr, W = 1e-4, 8
    for k in range(1, W + 1):
        assert tu.scheduled_lr(lr, k, W, "constant_with_warmup") == pytest.approx(lr * k / W, rel=1e-12)
    for k in (W, W + 1, 10 * W):
        assert tu.scheduled_lr(lr, k, W, "constant_with_warmup") == lr
    assert tu.scheduled_lr(lr, 1, 0, "constant_with_warmup") == lr
    for k in (1, W // 2, 10 * W):                      # get_scheduler("constant", ...) ignores the warm-up (the reference's setting)
        assert tu.scheduled_lr(lr, k, W, "constant") == lr
    with pytest.raises(ValueError):
        tu.scheduled_lr(lr, 1, W, "cosine")


def test_resume_picks_the_numerically_highest_checkpoint(tmp_path):
    d = str(tmp_path)
    assert tu.latest_checkpoint(d) is None and tu.latest_checkpoint(os.path.join(d, "missing")) is None
    for name in ("0009000.pt", "0010000.pt", "0010000.state.pt", "0010000.rng1.pt", "0009000.state.pt", "999999.pt", "notes.pt", "20000.txt"):
        open(os.path.join(d, name), "w").close()
    assert tu.latest_checkpoint(d) == os.path.join(d, "999999.pt")            # by number, not by name: "999999" > "0010000"
    os.remove(os.path.join(d, "999999.pt"))
    ck = tu.latest_checkpoint(d)
    assert ck == os.path.join(d, "0010000.pt") and tu.checkpoint_step(ck) == 10000
    assert tu.state_path(ck) == os.path.join(d, "0010000.state.pt") and tu.state_path(ck, 3) == os.path.join(d, "0010000.rng3.pt")
    assert tu.checkpoint_step(tu.state_path(ck)) is None


def test_micro_batch_data_index():
    seen = {}
    for step in range(1, 6):
        for micro in range(3):
            for rank in range(2):
                s = tu.data_seed(3407, step, micro, 3, rank, 2)
                assert s == tu.data_seed(3407, step, micro, 3, rank, 2)
                assert s not in seen, (seen[s], (step, micro, rank))
                seen[s] = (step, micro, rank)
    assert tu.data_seed(3408, 1, 0, 3, 0, 2) not in seen
    for step in (1, 7, 100000):                        # without accumulation: the index a run has always used
        for rank in range(4):
            assert tu.data_seed(3407, step, 0, 1, rank, 4) == 3407 * 1000003 + step * 4 + rank
    with pytest.raises(ValueError):
        tu.data_seed(1, 1, 3, 3, 0, 1)


def test_random_state_round_trip():
    torch.manual_seed(5)
    st = tu.rng_state()
    a = torch.rand(4)
    torch.rand(100)
    tu.set_rng_state(st)
    assert torch.equal(torch.rand(4), a)
