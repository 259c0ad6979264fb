"""Host-side pieces of the training driver (tools/train.py) that need no GPU: the learning-rate schedule, the data index of a
micro-batch, which checkpoint a resumed run continues from, and the random-state record that rides beside a checkpoint."""
import os
import re

import torch

STATE_SUFFIX = ".state.pt"     # <step>.pt is the reference's {"model", "ema"}; <step>.state.pt holds the rest of the run


def scheduled_lr(base_lr, step, warmup_steps=0, scheduler="constant"):
    """diffusers' ``get_scheduler(name, optimizer, num_warmup_steps)`` (train.py:169-173) for optimiser step ``step`` (from 1):
    "constant" ignores the warm-up, "constant_with_warmup" is linear from 0 over ``warmup_steps`` -- lr * k / W for k <= W, lr after."""
    if scheduler == "constant":
        return float(base_lr)
    if scheduler == "constant_with_warmup":
        w = int(warmup_steps or 0)
        return float(base_lr) * min(1.0, step / w) if w > 0 else float(base_lr)
    raise ValueError(f"lr_scheduler must be 'constant' or 'constant_with_warmup', got {scheduler!r}")


def clip_label(path):
    """The class label of a clip file: the ``<label>_...`` prefix of its name, 0 when it has none."""
    name = os.path.basename(path)
    return int(name.split("_")[0]) if name.split("_")[0].isdigit() else 0


def data_seed(seed, step, micro, accum, rank, world):
    """Seed of the data generator of micro-batch ``micro`` (0 .. accum-1) of optimiser step ``step`` on ``rank``: micro-batches are
    numbered step * accum + micro, ranks interleave inside one -- distinct for every (step, micro, rank), and step * world + rank
    (what a run without accumulation always used) for accum = 1."""
    if not (0 <= micro < accum and 0 <= rank < world):
        raise ValueError("need 0 <= micro < accum and 0 <= rank < world")
    return int(seed) * 1000003 + (int(step) * int(accum) + int(micro)) * int(world) + int(rank)


def resolve_loss_fn(spec):
    """The training config's ``loss_fn: "package.module:function"`` -> the callable ``LatteTrainer.train_step(loss_fn=...)`` takes
    (``loss_fn(model_out, x_start=, x_t=, t=, noise=) -> per-sample loss [B]``).  None / "" -> None: the built-in loss."""
    if spec in (None, ""):
        return None
    if not isinstance(spec, str) or spec.count(":") != 1 or not all(part.strip() for part in spec.split(":")):
        raise ValueError(f"loss_fn must be 'package.module:function', got {spec!r}")
    module, name = (part.strip() for part in spec.split(":"))
    import importlib
    try:
        mod = importlib.import_module(module)
    except ImportError as e:
        raise ValueError(f"loss_fn {spec!r}: cannot import module {module!r} ({e})") from e
    if not hasattr(mod, name):
        raise ValueError(f"loss_fn {spec!r}: module {module!r} has no attribute {name!r}")
    fn = getattr(mod, name)
    if not callable(fn):
        raise ValueError(f"loss_fn {spec!r}: {module}.{name} is not callable ({type(fn).__name__})")
    return fn


def latte_preset_name(name):
    """The model preset a training config's ``model:`` names: ``LatteIMG-XL/2`` (train_with_img.py, models/latte_img.py) has exactly the
    parameters of ``Latte-XL/2`` and its checkpoints are sampled with that preset, so the joint trainer runs on the plain model:
    "LatteIMG-<size>" -> "Latte-<size>"; every other name as it is (``get_models`` itself keeps refusing the LatteIMG names)."""
    name = str(name)
    return "Latte-" + name[len("LatteIMG-"):] if name.startswith("LatteIMG-") else name


def joint_loss_weights(num_frames, use_image_num):
    """(video, image) weights of the two passes of a joint micro-batch in its loss: mean_flat runs over all F + N frames of a sample,
    so the video pass carries F / (F + N) and the image pass N / (F + N)."""
    f, n = int(num_frames), int(use_image_num)
    if f < 1 or n < 0:
        raise ValueError("need num_frames >= 1 and use_image_num >= 0")
    return f / (f + n), n / (f + n)


def draw_image_frames(num_files, samples, use_image_num, generator):
    """Indices [samples, use_image_num] of the single frames that join each sample of a micro-batch, drawn with replacement from
    ``num_files`` files by the caller's seeded generator (data_seed): a resumed run redraws the same ones."""
    if num_files < 1 or samples < 1 or use_image_num < 1:
        raise ValueError("need num_files, samples and use_image_num >= 1")
    return torch.randint(0, int(num_files), (int(samples), int(use_image_num)), generator=generator)


def checkpoint_step(path):
    """0100000.pt -> 100000 (train.py:195-196); None for anything that is not a numbered checkpoint (the state files beside them)."""
    m = re.fullmatch(r"(\d+)\.pt", os.path.basename(str(path)))
    return int(m.group(1)) if m else None


def latest_checkpoint(ckpt_dir):
    """The numerically highest <step>.pt under ``ckpt_dir`` (train.py:180-192), or None."""
    if not os.path.isdir(ckpt_dir):
        return None
    found = [(checkpoint_step(f), f) for f in os.listdir(ckpt_dir)]
    found = [(s, f) for s, f in found if s is not None]
    return os.path.join(ckpt_dir, max(found)[1]) if found else None


def state_path(ckpt_path, rank=0):
    """The run-state file beside a checkpoint: rank 0's holds the optimiser state too, the other ranks' only their random state."""
    stem = str(ckpt_path)[:-len(".pt")]
    return stem + (STATE_SUFFIX if rank == 0 else f".rng{rank}.pt")


def rng_state(device=None):
    """torch's CPU and (current) device generator states of this process."""
    st = {"cpu": torch.get_rng_state()}
    if device is not None and torch.cuda.is_available():
        st["device"] = torch.cuda.get_rng_state(device)
    return st


def set_rng_state(st, device=None):
    torch.set_rng_state(st["cpu"].cpu().to(torch.uint8))
    if "device" in st and device is not None and torch.cuda.is_available():
        torch.cuda.set_rng_state(st["device"].cpu().to(torch.uint8), device)
