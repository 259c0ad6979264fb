"""Training on the engine: the body of the reference's optimisation loop (train.py:197-236) behind one object.

    trainer = LatteTrainer(model, diffusion, max_batch=5)          # model: latte_amd.Latte, diffusion: create_diffusion("")
    out = trainer.train_step(x_start, y=labels)                     # q_sample + forward + losses + backward + clip + AdamW + EMA
    trainer.ema_state_dict() / model.state_dict()                  # reference checkpoint format (train.py:257-262)
    out = trainer.forward(x_t, t, y); loss(out).backward(); trainer.optimizer_step()      # any torch loss; x_t.grad when asked for

What runs where: the forward with saved activations, the loss terms and their gradient, the backward (MFMA GEMMs for the
input / weight gradients, the attention backward, LayerNorm-modulate / GELU / gate backward kernels), gradient norm + clipping,
AdamW and the EMA update are engine kernels behind ``latte_trainer_*`` (include/latte_amd.h).  PyTorch holds the flat fp32
buffers (the model's ``nn.Parameter``s become views of the parameter buffer, as DistributedDataParallel's buckets do) and
averages the gradient buffer across ranks with ONE RCCL all-reduce per step when ``torch.distributed`` is initialised
(train.py:125 wraps the model in DDP; the engine itself never communicates).  There is no CPU / autograd fallback.
"""
import ctypes
import math

import torch

from . import _lib
from ._lib import LatteError, check, load_library, ptr, stream_ptr
from .diffusion import SpacedDiffusion, _LOSS
from .models import Latte

FROZEN = ("pos_embed", "temp_embed")   # nn.Parameter(requires_grad=False), latte.py:246-247
LORA_TARGETS = ("qkv", "proj", "fc1", "fc2")   # bit j of latte_trainer_lora_enable's target_mask
LORA_RANKS = (4, 8, 16, 32)   # rank 64 is refused: measured slower than the full step at Latte-B/2 (DESIGN.md 4.4 "LoRA")
SCALER_KEYS = ("loss_scale", "good_steps", "applied_updates", "skipped_updates", "last_skipped", "dynamic", "growth_interval", "max_scale")
_BUFFERS = ("params", "grads", "exp_avg", "exp_avg_sq", "ema")   # latte_trainer_bind's order


def lora_target_mask(targets):
    """("qkv", "fc2") -> the engine's target mask; a string "qkv,fc2" is accepted as the configs write it."""
    if isinstance(targets, str):
        targets = [t.strip() for t in targets.split(",") if t.strip()]
    targets = tuple(targets)
    bad = [t for t in targets if t not in LORA_TARGETS]
    if bad or not targets:
        raise LatteError(f"lora_targets must be a non-empty subset of {LORA_TARGETS}, got {list(targets)}")
    return sum(1 << LORA_TARGETS.index(t) for t in set(targets))


def _world(group=None):
    import torch.distributed as dist
    return dist.get_world_size(group) if dist.is_available() and dist.is_initialized() else 1


def average_gradients(flat_grads, group=None, async_op=False):
    """DistributedDataParallel's gradient averaging (train.py:125) as one all-reduce over a (slice of a) flat gradient buffer:
    RCCL over xGMI when the process group's backend is nccl, gloo in the CPU tests.  No-op without an initialised process group.
    async_op: returns the work handle (None when there is nothing to do); the caller divides by the world size after wait()."""
    import torch.distributed as dist
    world = _world(group)
    if world <= 1:
        return None if async_op else flat_grads
    if async_op:
        return dist.all_reduce(flat_grads, op=dist.ReduceOp.SUM, group=group, async_op=True)
    dist.all_reduce(flat_grads, op=dist.ReduceOp.SUM, group=group)
    flat_grads.div_(world)
    return flat_grads


def merge_lora_state_dict(sd, lora_sd, config):
    """A checkpoint's state dict with the adapters of ``lora_state_dict()`` folded in: W + (lora_alpha / lora_rank) B A in torch fp32
    for every ``<linear>.lora_A`` / ``.lora_B`` pair (``config``: ``lora_config()``).  For tools that have no trainer at hand
    (tools/sample.py --lora); ``LatteTrainer.merge_lora`` is the engine's own merge, whose fp32 sum may differ in the last bit."""
    s = float(config["lora_alpha"]) / int(config["lora_rank"])
    out = dict(sd)
    for k, a in lora_sd.items():
        if not k.endswith(".lora_A"):
            continue
        w, b = k[:-len(".lora_A")] + ".weight", lora_sd[k[:-1] + "B"]
        if w not in sd or tuple(sd[w].shape) != (b.shape[0], a.shape[1]):
            raise LatteError(f"merge_lora_state_dict: {k} does not fit {w}")
        out[w] = (sd[w].float() + s * (b.float().to(sd[w].device) @ a.float().to(sd[w].device))).to(sd[w].dtype)
    return out


class _FlatSet:
    """One trained set of the engine (the base, or the LoRA adapters) as PyTorch holds it: ``layout`` [(key, offset, numel)], the shape
    of every key and the five flat fp32 buffers the table lays out -- None for a buffer the set has none of (the frozen base of a
    LoRA trainer has ``params`` only).  family: "" reads latte_trainer_param_*, "lora_" reads latte_trainer_lora_param_*."""

    def __init__(self, h, family, shape_of, device, buffers=_BUFFERS):
        lib = load_library()
        fn = lambda name: getattr(lib, "latte_trainer_" + family + name)   # noqa: E731
        self.layout = [(fn("param_key")(h, i).decode(), int(fn("param_offset")(h, i)), int(fn("param_numel")(h, i)))
                       for i in range(fn("num_params")(h))]
        self.shapes = {k: tuple(shape_of(k)) for k, _, _ in self.layout}
        total = int(fn("total_numel")(h))
        for name in _BUFFERS:
            setattr(self, name, torch.zeros(total, device=device) if name in buffers else None)

    def pointers(self):
        return [ptr(getattr(self, name)) for name in _BUFFERS if getattr(self, name) is not None]

    def views(self, name):
        """{key: view of buffer ``name`` in the key's shape}"""
        flat = getattr(self, name)
        return {k: flat[off:off + numel].view(self.shapes[k]) for k, off, numel in self.layout}

    def keyed(self, name):
        return {k: v.clone() for k, v in self.views(name).items()}

    def load(self, name, sd, what=None):
        """``sd[key]`` of every key into buffer ``name``.  what (the caller's name in the messages): ``sd`` must hold exactly the set's
        keys in the set's shapes; without it further keys are ignored (a model's state dict also holds the frozen tables)."""
        if what:
            missing = [k for k in self.shapes if k not in sd]
            extra = [k for k in sd if k not in self.shapes]
            if missing or extra:
                raise LatteError(f"{what}: missing keys {missing[:4]}, unexpected keys {extra[:4]} (rank / targets differ?)")
            for k, shape in self.shapes.items():
                if tuple(sd[k].shape) != shape:
                    raise LatteError(f"{what}: {k} is {list(sd[k].shape)}, expected {list(shape)}")
        flat = getattr(self, name)
        with torch.no_grad():
            for k, off, numel in self.layout:
                flat[off:off + numel].copy_(sd[k].reshape(-1).float())


class _EngineDenoiser(torch.autograd.Function):
    """``LatteTrainer.forward`` as a node of the autograd graph: forward = latte_trainer_forward, backward = latte_trainer_seed + the
    backward stages (+ latte_trainer_input_grad).  ``anchor`` is a dummy that requires grad, so that the output carries a ``grad_fn``
    whether or not ``x`` does; nothing goes through ``save_for_backward`` -- the activations live in the engine."""

    @staticmethod
    def forward(ctx, x, anchor, trainer, t64, yy, generation):
        mo = trainer._engine_forward(x.detach(), t64, yy)
        ctx.trainer, ctx.generation, ctx.shape = trainer, generation, tuple(mo.shape)
        ctx.keep = (t64, yy)                       # the engine reads the labels until the last stage
        trainer._live = generation
        return mo

    @staticmethod
    def backward(ctx, grad):
        dx = ctx.trainer._engine_backward(ctx.generation, grad, ctx.shape, ctx.needs_input_grad[0])
        return dx, None, None, None, None, None


class LatteTrainer:
    """One data-parallel replica of train.py's model / ema / AdamW triple.

    lr, betas, eps, weight_decay: ``torch.optim.AdamW(model.parameters(), lr=1e-4, weight_decay=0)`` (train.py:127);
    clip_max_norm / start_clip_iter: train.py:228-231 (the gradient norm is always computed, clipping starts at that step);
    ema_decay: utils.update_ema's default; class_dropout_prob: LabelEmbedder's (latte.py:130), applied here because the engine
    takes the labels AFTER token_drop.
    compute_dtype: MFMA operand type of the forward / backward GEMMs and attention products; masters, gradients, AdamW state and
    EMA are fp32 either way.  "f16" runs the backward loss-scaled (``loss_scale``, a power of two, default 2**14: the per-token
    gradients of 1e-7 ... 1e-4 would underflow f16 otherwise; scaling and unscaling by a power of two is exact) and has the 10
    mantissa bits of the TF32 matmuls the reference trains with (train.py:12-14) -- the default: every gradient tensor within
    3.8e-4 relative L2 of the reference's fp32 gradients (tests/test_training_step.py); "bf16" needs no scaling, has 7 bits
    (3.2e-3) and is 1.6 % faster.
    Overflow handling (round 4): a non-finite gradient norm skips the update and, with ``dynamic_loss_scale`` (default: on for
    f16, off for bf16), halves the loss scale; 2000 applied updates in a row double it again -- all inside the engine's optimiser
    step, no host synchronisation (``scaler_state()`` reads the counters back for logging).  ``train_steps`` is the TRAINING-step
    counter of train.py:195-236 (clipping starts at ``start_clip_iter``, checkpoints are numbered by it, a continued run sets it to
    the checkpoint's step); AdamW's bias correction uses the engine's own count of applied updates, which starts at 0 with the
    fresh moments -- as ``torch.optim.AdamW`` does in the reference.
    gradient_accumulation_steps = A (train.py:222-236, accelerate's ``accumulate``): ``train_step`` runs ONE micro-batch; micro-batch 1
    of a window assigns the gradient buffer (no clear), micro-batches 2 .. A add to it inside the kernels that write it, the loss
    gradient is divided by A (the reported terms are not), and clip + AdamW + EMA run after the A-th -- ``train_steps`` counts those
    optimiser steps.  Data parallel: only the window's last micro-batch takes the staged backward with its per-stage all-reduce (of
    the ACCUMULATED slice, final only then); the earlier ones run without a collective, as under DDP's ``no_sync``.
    ``training_state()`` / ``load_training_state()`` carry everything a run is made of (parameters, EMA, AdamW moments, the eight
    loss-scale / update counters, ``train_steps``, a partial window) so that a resumed run continues bit for bit.
    use_image_num = N > 0: joint image-video training (train_with_img.py:214-241, models/latte_img.py, the ``*_img_train.yaml``
    configs): ``x_start`` is [B, F + N, C, H, W] -- F video frames and N single images per sample -- and class-conditional models take
    ``y_image`` [B, N] besides ``y``.  LatteIMG has exactly Latte's parameters and its image frames meet neither the video frames nor
    the temporal blocks, so the engine runs a joint micro-batch as the video step plus one spatial-only image pass over B N one-frame
    samples whose gradient writers add (include/latte_amd.h); the checkpoint is sampled with the plain ``Latte-*`` presets.  A joint
    micro-batch is ONE micro-batch of an accumulation window.  N <= num_frames; with N = 0 nothing changes.
    Custom losses: ``forward(x_t, t, y)`` returns the model output as a node of the torch autograd graph -- any torch loss of it calls
    ``backward()``, which seeds the engine's backward and fills ``x_t.grad`` -- and ``train_step(..., loss_fn=f)`` runs a whole step
    on ``f(model_out, x_start=, x_t=, t=, noise=) -> [B]``; diffusions with ``use_kl`` / ``predict_xstart`` train only that way.
    lora_rank = r > 0: LoRA fine-tuning (DESIGN.md 4.4 "LoRA").  The model's parameters are frozen; every targeted block linear
    (``lora_targets``, default all of qkv / proj / fc1 / fc2) runs with ``W + (lora_alpha / r) B A`` and only ``A [r, K]`` (kaiming-uniform,
    a = sqrt(5)) and ``B [N, r]`` (zero) train -- r in 4, 8, 16, 32; ``lora_alpha`` defaults to r.  No gradient, moment or EMA buffer of
    the base is allocated: ``grads`` / ``exp_avg`` / ``exp_avg_sq`` / ``ema`` are None and ``lora_params`` / ``lora_grads`` / ... take their
    place in every method (``lora_state_dict()`` is the small file to ship, ``merge_lora()`` turns the model into an ordinary
    checkpoint).  With lora_rank = 0 nothing changes and nothing is allocated."""

    def __init__(self, model, diffusion, max_batch, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, clip_max_norm=0.1,
                 start_clip_iter=20000, ema_decay=0.9999, class_dropout_prob=0.1, compute_dtype="f16", process_group=None,
                 loss_scale=None, dynamic_loss_scale=None, gradient_accumulation_steps=1, use_image_num=0, lora_rank=0, lora_alpha=None,
                 lora_targets=LORA_TARGETS):
        if not isinstance(model, Latte):
            raise LatteError("LatteTrainer needs a latte_amd.Latte model")
        if not isinstance(diffusion, SpacedDiffusion):
            raise LatteError("LatteTrainer needs a latte_amd SpacedDiffusion (create_diffusion)")
        if model.extras not in (1, 2):
            raise LatteError("T2V training are Not supported at this moment!")             # train.py:213-214
        if compute_dtype not in _lib.DTYPES:
            raise LatteError(f"compute_dtype must be one of {sorted(_lib.DTYPES)}")
        _lib.require_gpu()
        self.model, self.diffusion = model, diffusion
        self.max_batch = int(max_batch)
        self.lora_rank = int(lora_rank)
        self.lora_alpha = float(lora_alpha) if lora_alpha is not None else float(self.lora_rank)
        self.lora_targets = tuple(t for t in LORA_TARGETS if self.lora_rank and lora_target_mask(lora_targets) >> LORA_TARGETS.index(t) & 1)
        self.lora_merged = False
        if self.lora_rank and self.lora_rank not in LORA_RANKS:
            raise LatteError(f"lora_rank must be 0 or one of {LORA_RANKS}, got {self.lora_rank}")
        if self.lora_rank and not (self.lora_alpha > 0 and math.isfinite(self.lora_alpha)):
            raise LatteError("lora_alpha must be positive and finite")
        self.use_image_num = int(use_image_num)
        if self.use_image_num < 0:
            raise LatteError("use_image_num must be >= 0")
        if self.use_image_num > model.num_frames:
            raise LatteError(f"use_image_num {self.use_image_num} exceeds num_frames {model.num_frames}: the image pass runs in the "
                             "video pass's row buffers")
        if self.use_image_num and ((model.input_size // model.patch_size) ** 2) % 64:
            raise LatteError("joint image-video training needs (input_size / patch_size)^2 to be a multiple of 64")
        self.lr, self.betas, self.eps, self.weight_decay = float(lr), tuple(betas), float(eps), float(weight_decay)
        self.clip_max_norm, self.start_clip_iter, self.ema_decay = float(clip_max_norm), int(start_clip_iter), float(ema_decay)
        self.class_dropout_prob = float(class_dropout_prob)
        self.process_group = process_group
        self.always_staged = False     # test hook: take the staged (bucketed) backward path without a process group
        self.train_steps = 0
        self.gradient_accumulation_steps = int(gradient_accumulation_steps)
        if self.gradient_accumulation_steps < 1:
            raise LatteError("gradient_accumulation_steps must be >= 1")
        self.micro_step = 0            # micro-batches of the current window already in the gradient buffer
        self._generation = 0           # custom losses: the live ``forward`` (one graph at a time); 0 = none awaits its backward
        self._live = None
        self._accumulating = False     # the engine's "grad_accumulate" option as last set
        dev = next(model.parameters()).device
        if dev.type != "cuda":
            raise LatteError("move the model to the GPU first (model.to('cuda'))")
        self.device = dev
        lib = load_library()
        cfg = model.engine_config(compute_dtype)
        h = _lib.c_void()
        with torch.cuda.device(dev):
            if self.use_image_num:
                check(lib.latte_trainer_create_joint(cfg, self.max_batch, self.use_image_num, h))
            else:
                check(lib.latte_trainer_create(cfg, self.max_batch, h))
        self._h = h
        if self.lora_rank:
            check(lib.latte_trainer_lora_enable(h, self.lora_rank, self.lora_alpha, lora_target_mask(self.lora_targets)))
        if loss_scale is not None:
            check(lib.latte_trainer_set_option(h, b"loss_scale", float(loss_scale)))
        if dynamic_loss_scale is not None:
            check(lib.latte_trainer_set_option(h, b"dynamic_loss_scale", float(bool(dynamic_loss_scale))))
        if self.gradient_accumulation_steps != 1:
            check(lib.latte_trainer_set_option(h, b"loss_divisor", float(self.gradient_accumulation_steps)))
        self.compute_dtype = compute_dtype
        named = dict(model.named_parameters())
        lora = bool(self.lora_rank)
        # the base -- under LoRA frozen: parameters only, no gradient, moment or EMA buffer -- and the adapters; _trained: the set the
        # optimiser trains, whose buffers every step, state and collective below is about
        self._base = _FlatSet(h, "", lambda k: getattr(named.get(k), "shape", ()), dev, ("params",) if lora else _BUFFERS)
        if [k for k, _, _ in self._base.layout] != [k for k in named if k not in FROZEN]:
            raise LatteError("parameter order of the engine and of the model differ")
        self._linear_shapes = {k[:-len(".weight")]: tuple(p.shape) for k, p in named.items() if k.endswith(".weight") and p.dim() == 2}
        self._adapters = _FlatSet(h, "lora_", self.lora_shape, dev) if lora else None
        self._trained = self._adapters or self._base
        # the public names alias the sets' tensors: params / grads / exp_avg / exp_avg_sq / ema / layout, and lora_params ... lora_layout
        for prefix, fs in [("", self._base)] + ([("lora_", self._adapters)] if lora else []):
            for name in _BUFFERS + ("layout",):
                setattr(self, prefix + name, getattr(fs, name))
        with torch.no_grad():
            for k, p in self._base.views("params").items():
                p.copy_(named[k].detach().float())
                named[k].data = p                                              # the module's parameters are views of the flat buffer
            for k, a in self._adapters.views("params").items() if lora else ():
                if k.endswith(".lora_A"):                                      # nn.Linear's own init, as peft's LoRA layers; B stays 0
                    a.copy_(torch.nn.init.kaiming_uniform_(torch.empty(a.shape), a=math.sqrt(5)))
            self._trained.ema.copy_(self._trained.params)                      # update_ema(ema, model, decay=0), train.py:165
        with torch.cuda.device(dev):
            if lora:
                check(lib.latte_trainer_bind_lora(h, *self._base.pointers(), *self._adapters.pointers()))
            else:
                check(lib.latte_trainer_bind(h, *self._base.pointers()))
            check(lib.latte_trainer_set_frozen(h, ptr(named["pos_embed"].detach().float().contiguous()),
                                               ptr(named["temp_embed"].detach().float().contiguous()), 1, stream_ptr()))
            check(lib.latte_trainer_sync_weights(h, stream_ptr()))
        self._norm = torch.zeros(2, device=dev)
        self._anchor = torch.zeros((), device=dev, requires_grad=True)   # makes ``forward``'s output a node of the autograd graph
        self._weights_changed()

    def set_option(self, name, value):
        """Engine options of the trainer (latte_trainer_set_option): "loss_scale", "dynamic_loss_scale", "loss_scale_growth_interval",
        "fuse_gelu" (0: separate GELU passes, 1: inside the fc1 / fc2-gradient GEMMs -- the default), "fuse_small" (0: the
        separate finalize / column-sum / adaLN / gate-backward launches of rounds 2 - 6, 1: folded -- the default, csrc/train_fin.hip;
        not while a step is in flight), "grad_accumulate" / "loss_divisor" (what ``gradient_accumulation_steps`` drives; see
        include/latte_amd.h)."""
        check(load_library().latte_trainer_set_option(self._h, name.encode(), float(value)))

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                load_library().latte_trainer_destroy(self._h)
        except Exception:
            pass

    # ------------------------------------------------------------------ views
    def grad_dict(self):
        """{reference key: gradient view} of the last forward_backward."""
        if self.lora_rank:
            raise LatteError("a LoRA trainer has no base gradients: lora_grad_dict()")
        return self._base.views("grads")

    def _weights_changed(self):
        if hasattr(self.model, "mark_weights_dirty"):
            self.model.mark_weights_dirty()

    # ------------------------------------------------------------------ LoRA
    def lora_shape(self, key):
        """Shape of adapter ``key``: lora_A [r, in_features], lora_B [out_features, r] of the linear it belongs to."""
        n, k = self._linear_shapes[key.rsplit(".", 1)[0]]
        return (self.lora_rank, k) if key.endswith(".lora_A") else (n, self.lora_rank)

    def _need_lora(self):
        if not self.lora_rank:
            raise LatteError("this trainer was built without LoRA (lora_rank=0)")

    def lora_state_dict(self):
        """{``blocks.{i}.attn.qkv.lora_A``: [r, K], ``....lora_B``: [N, r], ...} of the targeted linears: the file a fine-tune ships
        (with ``lora_config()`` beside it)."""
        self._need_lora()
        return self._adapters.keyed("params")

    def ema_lora_state_dict(self):
        self._need_lora()
        return self._adapters.keyed("ema")

    def lora_grad_dict(self):
        """{adapter key: gradient view} of the last backward."""
        self._need_lora()
        return self._adapters.views("grads")

    def lora_config(self):
        return {"lora_rank": self.lora_rank, "lora_alpha": self.lora_alpha, "lora_targets": list(self.lora_targets)}

    def load_lora_state_dict(self, sd, ema_sd=None):
        """Adapters (and their EMA: ``ema_sd``, default the adapters themselves) back into the flat buffers; the merged operand copies
        are re-packed."""
        self._need_lora()
        self._not_merged()
        self._adapters.load("params", sd, "load_lora_state_dict")
        self._adapters.load("ema", ema_sd or sd, "load_lora_state_dict")
        with torch.cuda.device(self.device):
            check(load_library().latte_trainer_sync_weights(self._h, stream_ptr()))

    def _not_merged(self):
        if self.lora_merged:
            raise LatteError("merge_lora() folded the adapters into the model: this trainer is finished, build a new one to go on")

    def merge_lora(self, ema=False):
        """Writes ``W + (alpha / r) B A`` (``ema``: of the EMA adapters) into the model's parameters through the engine's merge entry --
        the pack's fp32 arithmetic, so a plain trainer or the sampling engine on the merged model runs the operands this trainer ran.
        ``model.state_dict()`` is an ordinary checkpoint afterwards; this trainer is finished (its base now holds the adapters)."""
        self._need_lora()
        self._not_merged()
        if self.micro_step:
            raise LatteError("merge_lora inside an accumulation window")
        self._live = None
        with torch.cuda.device(self.device):
            check(load_library().latte_trainer_lora_merge(self._h, ptr(self.lora_ema) if ema else None, ptr(self.params), stream_ptr()))
        self.lora_merged = True
        self._weights_changed()
        return self.model

    def model_state_dict(self):
        """The ``"model"`` entry of train.py's checkpoints (:257-262), built from the flat fp32 master buffer through the layout --
        not through the module's parameter views: a later ``model.cuda()`` / ``.to()`` / ``.float()`` re-materialises the
        ``nn.Parameter``s and silently ends the aliasing, after which ``model.state_dict()`` would be stale."""
        return {**{k: v.detach().clone() for k, v in self.model.state_dict().items()}, **self._base.keyed("params")}

    def check_aliasing(self):
        """True while every trained ``nn.Parameter`` of the module still is a view of the flat master buffer."""
        named = dict(self.model.named_parameters())
        base = self.params.data_ptr()
        return all(named[k].data_ptr() == base + 4 * off for k, off, _ in self.layout)

    def ema_state_dict(self):
        """The ``"ema"`` entry of train.py's checkpoints (:257-262): every key of model.state_dict()."""
        ema = self._base.keyed("params" if self.lora_rank else "ema")            # LoRA: the base is frozen, its average is itself
        return {**{k: v.detach().clone() for k, v in self.model.state_dict().items()}, **ema}

    def load_state_dict(self, sd, ema_sd=None):
        self._not_merged()
        self._base.load("params", sd)
        if not self.lora_rank:
            self._base.load("ema", ema_sd or sd)
        with torch.cuda.device(self.device):
            check(load_library().latte_trainer_sync_weights(self._h, stream_ptr()))

    # ------------------------------------------------------------------ one iteration of train.py:197-236
    def _image_labels(self, y_image, B, image_drop_mask):
        """y_image: [B, N] tensor or the reference's list of B tensors of N labels (train_with_img.py:218-221) -> int64 [B, N] on the
        device after the images' label dropout: ONE coin per sample for all of its images (latte_img.py:341-342 reshapes a sample's
        image labels to [1, N] and token_drop draws rand(labels.shape[0]))."""
        if y_image is None:
            raise LatteError("class-conditional model with use_image_num: y_image (the images' labels) required")
        if isinstance(y_image, (list, tuple)):
            y_image = torch.stack([torch.as_tensor(v).reshape(-1) for v in y_image])
        yi = y_image.to(device=self.device, dtype=torch.int64)
        if tuple(yi.shape) != (B, self.use_image_num):
            raise LatteError(f"y_image must be [batch, use_image_num] = [{B}, {self.use_image_num}], got {list(yi.shape)}")
        if image_drop_mask is not None:
            yi = torch.where(image_drop_mask.to(self.device).reshape(B, 1), torch.full_like(yi, self.model.num_classes), yi)
        if int(yi.min()) < 0 or int(yi.max()) > self.model.num_classes:
            raise IndexError("label out of range")
        return yi.contiguous()

    def forward_backward(self, x_start, t, noise, y=None, drop_mask=None, return_model_out=False, overlap_all_reduce=False,
                         y_image=None, image_drop_mask=None):
        """q_sample + forward + training_losses + backward; gradients of ``terms['loss'].mean()`` land in ``self.grads``
        (overlap_all_reduce: already averaged over the process group, bucket by bucket under the backward).
        A trainer with ``use_image_num`` = N takes the joint micro-batch [B, F + N, C, H, W] (and ``y_image`` / ``image_drop_mask``);
        a micro-batch of F frames still takes the plain step.
        -> dict(loss, mse, vb [, model_out])."""
        self._reduced = False
        self._live = None                                                          # a custom ``forward`` awaiting its backward is abandoned
        self._not_merged()
        d = self.diffusion
        self._builtin_loss_check()
        x0, nz, t64 = self._on_device(x_start, noise, t)
        B = x0.shape[0]
        if B > self.max_batch:
            raise LatteError(f"batch {B} exceeds max_batch {self.max_batch}")
        F, N = self.model.num_frames, self.use_image_num
        if N and (x0.dim() != 5 or x0.shape[1] not in (F, F + N)):
            raise LatteError(f"x_start must be [batch, {F + N} (or {F}: video only), C, H, W], got {list(x0.shape)}")
        joint = N > 0 and x0.shape[1] == F + N
        if nz.shape != x0.shape:
            raise AssertionError("noise.shape == x_start.shape")
        yy = self._labels(y, drop_mask)
        terms = torch.empty(3, B, device=self.device)
        mo = torch.empty(B, x0.shape[1], self.model.out_channels, x0.shape[3], x0.shape[4], device=self.device) if return_model_out else None
        lib = load_library()
        args = (self._h, d._h, _LOSS[d.loss_type], ptr(x0), ptr(nz), ptr(t64), ptr(yy) if yy is not None else None, B, ptr(terms),
                ptr(mo) if mo is not None else None, stream_ptr())
        run, begin = lib.latte_trainer_forward_backward, lib.latte_trainer_begin
        if joint:
            yi = self._image_labels(y_image, B, image_drop_mask) if self.model.extras == 2 else None
            self._y_image = yi                                     # alive until the last stage
            args = args[:7] + (ptr(yi), B, N) + args[8:]
            run, begin = lib.latte_trainer_forward_backward_joint, lib.latte_trainer_begin_joint
        with torch.cuda.device(self.device):
            if not overlap_all_reduce:
                check(run(*args))
            else:
                # bucketed data parallelism: as soon as a stage's gradient slice is final its all-reduce is enqueued (RCCL runs it
                # on its own stream behind the kernels already launched) while the next stages' kernels follow on this stream
                # (a joint micro-batch: the video pass ran inside begin, these are the image pass's stages -- final slices)
                check(begin(*args))
                self._run_stages(True)
        out = {"loss": terms[0], "mse": terms[1]}
        if d.learn_sigma:
            out["vb"] = terms[2]
        if mo is not None:
            out["model_out"] = mo
        return out

    def _builtin_loss_check(self):
        d = self.diffusion
        if d.loss_type not in ("mse", "rescaled_mse"):
            raise LatteError("the engine's built-in loss is one of the MSE loss types (create_diffusion's default and "
                             "rescale_learned_sigmas); pass loss_fn= for anything else")
        if d.predict_xstart:
            raise LatteError("the engine's built-in loss trains the epsilon-prediction models of train.py:92; pass loss_fn= for a "
                             "predict_xstart diffusion")

    def _run_stages(self, reduce):
        """The backward stages behind a begin / seed, in order.  reduce: each stage's finished gradient slice is all-reduced while
        the next stages run (no-op without a process group) and the trained set's ``grads`` leaves here averaged.  Adapters are
        megabytes of gradients: they take one collective behind the last stage instead (all_reduce_gradients)."""
        lib = load_library()
        grads, per_stage, handles = self._trained.grads, reduce and not self.lora_rank, []
        for k in range(lib.latte_trainer_num_stages(self._h)):
            check(lib.latte_trainer_backward_stage(self._h, k, stream_ptr()))
            if not per_stage:
                continue
            off, n = _lib.c_i64(), _lib.c_i64()
            check(lib.latte_trainer_stage_range(self._h, k, off, n))
            h = average_gradients(grads[off.value:off.value + n.value], self.process_group, async_op=True)
            if h is not None:
                handles.append(h)
        for h in handles:
            h.wait()
        if handles:
            grads.div_(_world(self.process_group))
        if per_stage:
            self._reduced = True
        elif reduce:
            self.all_reduce_gradients()

    def _on_device(self, x_start, noise, t):
        """-> x_start and noise as float32, t as int64: on the trainer's device, contiguous"""
        return (x_start.to(device=self.device, dtype=torch.float32).contiguous(),
                noise.to(device=self.device, dtype=torch.float32).contiguous(), t.to(device=self.device, dtype=torch.int64).contiguous())

    def _staged(self, last):
        """A window's last micro-batch takes the staged, all-reducing backward when there is a process group (or the test hook)."""
        return last and (_world(self.process_group) > 1 or self.always_staged)

    def _end_micro_batch(self, last):
        self.micro_step += 1
        if last:
            self.all_reduce_gradients()

    # ------------------------------------------------------------------ custom losses: forward / backward through torch.autograd
    def _labels(self, y, drop_mask):
        """-> the labels the engine takes: int64 on the device, after label dropout; None without a label table."""
        if self.model.extras != 2:
            return None
        if y is None:
            raise LatteError("class-conditional model: labels required")
        yy = y.to(device=self.device, dtype=torch.int64)
        if drop_mask is not None:                                                  # LabelEmbedder.token_drop, latte.py:138-148
            yy = torch.where(drop_mask.to(self.device), torch.full_like(yy, self.model.num_classes), yy)
        if int(yy.min()) < 0 or int(yy.max()) > self.model.num_classes:
            raise IndexError("label out of range")
        return yy.contiguous()

    def forward(self, x, t, y=None, drop_mask=None):
        """``model(x, t, y)`` on the engine with saved activations: x [B, F, C, H, W] the (noised) model input, t [B] the ORIGINAL
        timesteps the model sees (``diffusion.timestep_map[t]`` of a respaced index), y labels (``drop_mask``: label dropout applied
        here).  -> model_out [B, F, C_out, H, W] fp32 with a ``grad_fn``: any torch loss of it can call ``backward()``, which seeds the
        engine's staged backward with the incoming gradient.  Parameter gradients land in the flat ``self.grads`` (assigned by the
        window's first micro-batch, added by the others, divided by ``gradient_accumulation_steps``, all-reduced after the last --
        exactly as ``backward_micro_batch``'s), NOT in ``param.grad``; ``x.grad`` is filled when ``x.requires_grad``.  The backward
        counts as one micro-batch of the window: ``optimizer_step()`` is due after the ``gradient_accumulation_steps``-th.
        One graph is alive at a time: a newer ``forward`` (or a built-in step) makes this output's backward a ``LatteError``, as is
        a second backward.  Under ``torch.no_grad()`` the output is a plain tensor.  The loss-scaled f16 backward multiplies the
        incoming gradient by the live loss scale (2**14 by default): see DESIGN.md 4.4 before seeding it with a loss whose gradient
        is orders of magnitude away from the built-in one's."""
        if self.micro_step >= self.gradient_accumulation_steps:
            raise LatteError("the accumulation window is complete: optimizer_step() is due")
        self._not_merged()
        Fr, C, H = self.model.num_frames, self.model.in_channels, self.model.input_size
        if not torch.is_tensor(x) or x.dim() != 5 or tuple(x.shape[1:]) != (Fr, C, H, H):
            raise LatteError(f"forward: x must be [batch, {Fr}, {C}, {H}, {H}], got {list(getattr(x, 'shape', []))}"
                             + (" (a joint F + N micro-batch has no custom-loss path)" if self.use_image_num else ""))
        B = x.shape[0]
        if B < 1 or B > self.max_batch:
            raise LatteError(f"batch {B} exceeds max_batch {self.max_batch}")
        if x.device != self.device and x.requires_grad:
            raise LatteError("forward: an input that requires grad must live on the trainer's device")
        t64 = t.to(device=self.device, dtype=torch.int64).contiguous()
        if tuple(t64.shape) != (B,):
            raise LatteError(f"forward: t must be [{B}], got {list(t64.shape)}")
        yy = self._labels(y, drop_mask)
        if yy is not None and tuple(yy.shape) != (B,):
            raise LatteError(f"forward: y must be [{B}], got {list(yy.shape)}")
        self._reduced = False
        self._live = None
        self._set_accumulate(self.micro_step > 0)
        self._generation += 1
        if not torch.is_grad_enabled():
            return self._engine_forward(x.detach(), t64, yy)
        return _EngineDenoiser.apply(x, self._anchor, self, t64, yy, self._generation)

    def _engine_forward(self, x, t64, yy):
        x32 = x.to(device=self.device, dtype=torch.float32).contiguous()
        mo = torch.empty(x32.shape[0], x32.shape[1], self.model.out_channels, x32.shape[3], x32.shape[4], device=self.device)
        with torch.cuda.device(self.device):
            check(load_library().latte_trainer_forward(self._h, ptr(x32), ptr(t64), ptr(yy) if yy is not None else None, x32.shape[0],
                                                       ptr(mo), stream_ptr()))
        return mo

    def _engine_backward(self, generation, grad, shape, want_dx):
        if self._live != generation:
            raise LatteError("backward of a LatteTrainer.forward output that is no longer alive: one graph at a time, one backward per "
                             "forward (a newer forward or a built-in step came in between, or this is a second backward)")
        if (not torch.is_tensor(grad) or tuple(grad.shape) != tuple(shape) or grad.dtype != torch.float32 or grad.device != self.device):
            raise LatteError(f"backward: the gradient of model_out must be float32 {list(shape)} on {self.device}, got "
                             f"{getattr(grad, 'dtype', None)} {list(getattr(grad, 'shape', []))} on {getattr(grad, 'device', None)}")
        self._live = None
        g = grad.contiguous()
        last = self.micro_step == self.gradient_accumulation_steps - 1
        lib = load_library()
        dx = None
        with torch.cuda.device(self.device):
            check(lib.latte_trainer_seed(self._h, ptr(g), stream_ptr()))
            self._run_stages(self._staged(last))
            if want_dx:
                dx = torch.empty(shape[0], shape[1], self.model.in_channels, shape[3], shape[4], device=self.device)
                check(lib.latte_trainer_input_grad(self._h, ptr(dx), stream_ptr()))
                if self.gradient_accumulation_steps != 1:       # the engine's gradients are those of loss / A; x.grad is the loss's own
                    dx.mul_(float(self.gradient_accumulation_steps))
        self._end_micro_batch(last)
        return dx

    def all_reduce_gradients(self):
        """DDP's gradient averaging (train.py:125) as ONE collective over the flat gradient buffer: RCCL over xGMI when the
        process group's backend is nccl, gloo in the CPU tests."""
        if not getattr(self, "_reduced", False):
            average_gradients(self._trained.grads, self.process_group)
            self._reduced = True

    def _set_accumulate(self, on):
        if on != self._accumulating:
            check(load_library().latte_trainer_set_option(self._h, b"grad_accumulate", float(on)))
            self._accumulating = on

    def backward_micro_batch(self, x_start, t, noise, y=None, drop_mask=None, y_image=None, image_drop_mask=None, loss_fn=None):
        """The next micro-batch of the accumulation window: ``forward_backward`` in assign mode for the first, in accumulate mode
        for the others; the window's last one takes the staged, all-reducing backward when there is a process group.
        loss_fn: a callable ``loss_fn(model_out, x_start=, x_t=, t=, noise=) -> per-sample loss [B]`` in torch replaces the built-in
        loss: q_sample by the engine's kernel, ``forward``, ``loss_fn(...).mean().backward()`` (t: the respaced indices).
        -> (forward_backward's dict -- with a loss_fn: {"loss": per-sample loss} --, True when the window is complete and
        ``optimizer_step`` is due)."""
        if self.micro_step >= self.gradient_accumulation_steps:
            raise LatteError("the accumulation window is complete: optimizer_step() is due")
        last = self.micro_step == self.gradient_accumulation_steps - 1
        if loss_fn is not None:
            if not callable(loss_fn):
                raise LatteError("loss_fn must be callable")
            if y_image is not None or (torch.is_tensor(x_start) and x_start.dim() == 5 and x_start.shape[1] != self.model.num_frames):
                raise LatteError("custom losses take video micro-batches of num_frames frames: no joint image-video pass")
            d = self.diffusion
            x0, nz, t64 = self._on_device(x_start, noise, t)
            x_t = d.q_sample(x0, t64, nz)
            t_model = torch.tensor(d.timestep_map, device=self.device, dtype=torch.int64)[t64]
            with torch.enable_grad():
                out = self.forward(x_t, t_model, y, drop_mask)
                per_sample = loss_fn(out, x_start=x0, x_t=x_t, t=t64, noise=nz)
                if not torch.is_tensor(per_sample) or tuple(per_sample.shape) != (x0.shape[0],):
                    raise LatteError(f"loss_fn must return the per-sample loss [{x0.shape[0]}], got {list(getattr(per_sample, 'shape', []))}")
                per_sample.mean().backward()
            if self._live is not None:                                             # no gradient reached the engine: no micro-batch ran
                self._live = None
                raise LatteError("loss_fn's result does not depend on model_out")
            return {"loss": per_sample.detach()}, last
        self._set_accumulate(self.micro_step > 0)
        out = self.forward_backward(x_start, t, noise, y, drop_mask, overlap_all_reduce=self._staged(last), y_image=y_image,
                                    image_drop_mask=image_drop_mask)
        self._end_micro_batch(last)
        return out, last

    def optimizer_step(self):
        """clip_grad_norm_ + AdamW + update_ema; -> gradient norm (0-d tensor, device).  Ends the accumulation window."""
        self._not_merged()
        self.micro_step = 0
        self._set_accumulate(False)     # a plain forward_backward assigns again
        self.train_steps += 1
        clip = int(self.train_steps - 1 >= self.start_clip_iter)                  # train.py:228-231
        with torch.cuda.device(self.device):
            # step = 0: AdamW's bias correction counts the engine's APPLIED updates (fresh moments start at 1), not train_steps
            check(load_library().latte_trainer_optimizer_step(self._h, self.lr, self.betas[0], self.betas[1], self.eps, self.weight_decay,
                                                              0, self.clip_max_norm, clip, self.ema_decay,
                                                              ptr(self._norm), stream_ptr()))
        self._weights_changed()
        return self._norm[0]

    def scaler_state(self):
        """Loss-scaling / update counters of the engine (synchronises): dict(loss_scale, good_steps, applied_updates,
        skipped_updates, last_skipped, dynamic, growth_interval, max_scale)."""
        out = (ctypes.c_double * 8)()
        check(load_library().latte_trainer_scaler_state(self._h, out))
        return dict(zip(SCALER_KEYS, [float(v) for v in out]))

    def set_scaler_state(self, state):
        """Puts the eight values of ``scaler_state()`` back (latte_trainer_set_scaler_state)."""
        check(load_library().latte_trainer_set_scaler_state(self._h, (ctypes.c_double * 8)(*[float(state[k]) for k in SCALER_KEYS])))

    # ------------------------------------------------------------------ the whole state of a run
    def _state_slots(self, state):
        """Where the trained set's entries live in a ``training_state()`` dict: -> (the dict of the moments ``exp_avg`` /
        ``exp_avg_sq``, the dict of the partial gradient buffer ``grads``)."""
        return (state["lora"], state["lora"]) if self.lora_rank else (state["opt"], state)

    def training_state(self):
        """Everything a run continues from: ``model`` / ``ema`` (the reference's checkpoint entries, train.py:257-262), ``opt``
        (AdamW's ``exp_avg`` / ``exp_avg_sq``, state-dict keyed), ``scaler`` (the eight counters), ``train_steps``, ``micro_step``
        and, inside a window (``micro_step != 0``), the partial gradient buffer ``grads``.  A LoRA trainer: the frozen base once as
        ``model`` (its EMA is itself, it has no moments), and under ``lora`` everything of the adapters -- ``config``, ``params``,
        ``ema``, the moments and the partial gradients."""
        st = {"model": self.model_state_dict()}
        if self.lora_rank:
            st["lora"] = {"config": self.lora_config(), "params": self.lora_state_dict(), "ema": self.ema_lora_state_dict()}
        else:
            st["ema"], st["opt"] = self.ema_state_dict(), {}
        st.update(scaler=self.scaler_state(), train_steps=int(self.train_steps), micro_step=int(self.micro_step),
                  gradient_accumulation_steps=int(self.gradient_accumulation_steps))
        moments, partial = self._state_slots(st)
        moments.update(exp_avg=self._trained.keyed("exp_avg"), exp_avg_sq=self._trained.keyed("exp_avg_sq"))
        if self.micro_step:
            partial["grads"] = self._trained.keyed("grads")
        return st

    def load_training_state(self, state):
        """The inverse of ``training_state()``: buffers, counters and window position back, the packed weights re-synced."""
        micro = int(state.get("micro_step", 0))
        if micro and int(state.get("gradient_accumulation_steps", self.gradient_accumulation_steps)) != self.gradient_accumulation_steps:
            raise LatteError("the state was saved inside an accumulation window of another gradient_accumulation_steps")
        if bool(self.lora_rank) != ("lora" in state):
            raise LatteError("the state and the trainer disagree on LoRA")
        if self.lora_rank and state["lora"]["config"] != self.lora_config():
            raise LatteError(f"the state's adapters are {state['lora']['config']}, the trainer's {self.lora_config()}")
        moments, partial = self._state_slots(state)
        if micro and "grads" not in partial:
            raise LatteError("the state was saved inside an accumulation window but holds no gradients")
        self._trained.load("exp_avg", moments["exp_avg"])
        self._trained.load("exp_avg_sq", moments["exp_avg_sq"])
        if micro:
            self._trained.load("grads", partial["grads"])
        else:
            self._trained.grads.zero_()
        if self.lora_rank:                                                 # (both branches sync the packed operand copies)
            self._base.load("params", state["model"])
            self.load_lora_state_dict(state["lora"]["params"], state["lora"]["ema"])
        else:
            self.load_state_dict(state["model"], state["ema"])
        self.set_scaler_state(state["scaler"])
        self.train_steps, self.micro_step = int(state["train_steps"]), micro
        self._weights_changed()

    def train_step(self, x_start, y=None, t=None, noise=None, drop_mask=None, y_image=None, image_drop_mask=None, loss_fn=None):
        """train.py:197-236 for one micro-batch; the optimiser step runs after the ``gradient_accumulation_steps``-th of a window
        (``out["updated"]``; ``out["grad_norm"]`` only then).  loss_fn: the caller's loss in torch instead of the built-in one
        (``backward_micro_batch``); diffusions with ``use_kl`` / ``predict_xstart`` are accepted only with one."""
        B = x_start.shape[0]
        if t is None:
            t = torch.randint(0, self.diffusion.num_timesteps, (B,), device=self.device)       # train.py:223
        if noise is None:
            noise = torch.randn_like(x_start, dtype=torch.float32, device=self.device)          # gd:733-734
        if drop_mask is None and self.model.extras == 2 and self.class_dropout_prob > 0:
            drop_mask = torch.rand(B, device=self.device) < self.class_dropout_prob              # latte.py:142-143
        if (image_drop_mask is None and y_image is not None and self.use_image_num and self.model.extras == 2
                and self.class_dropout_prob > 0):
            image_drop_mask = torch.rand(B, device=self.device) < self.class_dropout_prob        # latte_img.py:341-342: one coin per sample
        out, last = self.backward_micro_batch(x_start, t, noise, y, drop_mask, y_image, image_drop_mask, loss_fn=loss_fn)
        out["updated"] = last
        if last:
            out["grad_norm"] = self.optimizer_step()
        return out
