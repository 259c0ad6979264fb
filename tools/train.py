"""train.py of the reference, re-hosted on the MI355X engine (BASELINE config 5).

  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 tools/train.py --config configs/ffs_train.yaml
  python tools/train.py --config configs/ffs_train.yaml --max-steps 20 --log-every 5          (single GPU)

One process per GPU (train.py:55-66), the model replicated, `local_batch_size` latent clips per rank and step; per step
`LatteTrainer.train_step` = q_sample + forward + training_losses + backward (gradient slices all-reduced over RCCL bucket by bucket
under the backward) + clip_grad_norm_ + AdamW + update_ema (train.py:197-236).  `gradient_accumulation_steps: A` draws A
micro-batches per optimiser step (steps, logs and checkpoints count optimiser steps).  Checkpoints are the reference's
`{"model": state_dict, "ema": state_dict}` (train.py:257-262) and load back through `find_model` / `pretrained:`; beside each,
`<step>.state.pt` holds the rest of the run (AdamW moments, loss-scale / update counters, step, random states; ranks > 0 write
`<step>.rng<rank>.pt`), and `resume_from_checkpoint: True` continues from the highest-numbered pair bit for bit.
`data_path` holds one of
  - uint8 frame clips (.npy [F, H, W, 3], H == W == image_size): every batch is encoded on the GPU as the reference does
    (train.py:204-211, `vae.encode(x).latent_dist.sample().mul_(0.18215)`) through `AutoencoderKL.encode_video_uint8`, the VAE
    loaded from `<pretrained_model_path>/vae` with the encoder (train.py:94), fresh posterior noise every step from a seeded generator;
  - latent clips (.npy [F, 4, h, w], already scaled by 0.18215; tools/encode_clips.py writes them from frame clips once, instead of
    encoding every epoch);
  - "synthetic" (N(0, 1) latents: throughput and plumbing, not a model worth keeping);
  - with `frame_interval` set in the config (the reference's key, configs/tiny_train_raw.yaml): RAW uint8 clips (.npy [T, Hs, Ws, 3] of any
    length and size, memory-mapped), read as the reference's dataset classes read a video (datasets/ucf101_datasets.py:198-216): per item
    and step a `TemporalRandomCrop(num_frames * frame_interval)` window and the flip coin from a seeded generator, the `num_frames` frames
    of `frame_indices` gathered on the host, one upload, one `latte_amd.video_transforms` launch for `dataset`'s pipeline
    (ffs | ucf101 | taichi | sky), then the encode above -- nothing of the augmentation is frozen into the stored data.
`moments_path` (with `frame_interval`; configs/tiny_train_moments.yaml) replaces `data_path` by the stored VAE moments of those raw
clips (tools/encode_clips.py --moments; latte_amd.MomentStore): the same window, flip and posterior-noise draws as the raw mode for the
same seed, served by one gather-and-sample launch per micro-batch -- no VAE is loaded.  `frame_moments_path` does the same for the single
images of `use_image_num`; `--moments-device cpu` keeps the stores in host memory.
Joint image-video training (train_with_img.py, the `*_img_train.yaml` configs): `use_image_num: N` appends N single frames to every
clip and `model: LatteIMG-*` is mapped to the `Latte-*` preset of the same size (identical parameters; the checkpoint is sampled with
it).  `frame_data_path` is a directory of single frames -- .npy latents [4, h, w] (scaled by 0.18215) or uint8 [H, W, 3] at the
training image size, encoded with the VAE like the frame clips; label = file-name prefix, as for clips -- N of them drawn per sample
from the micro-batch's seeded generator (a resumed run redraws the same ones); with `data_path: synthetic` they are synthetic too.
`loss_fn: "package.module:function"` replaces the built-in loss by a torch one (`LatteTrainer.train_step(loss_fn=...)`:
`function(model_out, x_start=, x_t=, t=, noise=) -> per-sample loss [B]`, differentiated through `LatteTrainer.forward`); video
micro-batches only (not with `use_image_num`).
LoRA fine-tuning (`lora_rank: r` with `pretrained:`; `lora_alpha`, default r; `lora_targets`, default "qkv,proj,fc1,fc2"): the checkpoint
named by `pretrained:` stays frozen and rank-r adapters on the targeted block linears train (LatteTrainer(lora_rank=...)).  A
checkpoint then is `<step>.lora.pt` = {"config", "lora", "lora_ema"} -- megabytes; the base is not written again -- with the same
`<step>.state.pt` / `<step>.rng<rank>.pt` beside it, and `resume_from_checkpoint: True` continues from the highest-numbered one bit for
bit.  `tools/sample.py --ckpt <pretrained> --lora <step>.lora.pt` samples the fine-tune.
"""
import argparse
import glob
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import latte_amd  # noqa: E402
from latte_amd import parallel  # noqa: E402
from latte_amd.train_util import (checkpoint_step, clip_label, data_seed, draw_image_frames, latest_checkpoint, latte_preset_name,  # noqa: E402
                                  resolve_loss_fn, rng_state, scheduled_lr, set_rng_state, state_path)


def latest_lora_checkpoint(ckpt_dir):
    """The numerically highest <step>.lora.pt under ``ckpt_dir``, or None."""
    import re
    found = [(int(m.group(1)), f) for f in (os.listdir(ckpt_dir) if os.path.isdir(ckpt_dir) else [])
             for m in [re.fullmatch(r"(\d+)\.lora\.pt", f)] if m]
    return os.path.join(ckpt_dir, max(found)[1]) if found else None


def _cpu(d):
    return {k: v.cpu() for k, v in d.items()}


def split_run_state(trainer_state, lora):
    """``LatteTrainer.training_state()`` as a run directory holds it -> (checkpoint file name suffix, checkpoint payload, state-file
    payload).  The checkpoint is the file to ship: ``<step>.pt`` = the reference's {model, ema}, or with ``lora`` ``<step>.lora.pt`` =
    {config, lora, lora_ema} (the frozen base stays the `pretrained:` file).  The state file takes the rest: the AdamW moments (``opt``,
    or ``lora_opt``) and the counters; main() adds the random state."""
    st = trainer_state
    if lora:
        lo = st["lora"]
        rest = {k: v for k, v in st.items() if k not in ("model", "lora")}
        rest["lora_opt"] = {m: _cpu(lo[m]) for m in ("exp_avg", "exp_avg_sq")}
        return ".lora.pt", {"config": lo["config"], "lora": _cpu(lo["params"]), "lora_ema": _cpu(lo["ema"])}, rest
    rest = {k: v for k, v in st.items() if k not in ("model", "ema", "opt")}
    rest["opt"] = {m: _cpu(st["opt"][m]) for m in st["opt"]}
    return ".pt", {"model": _cpu(st["model"]), "ema": _cpu(st["ema"])}, rest


def join_run_state(checkpoint, state, lora, base_model=None):
    """The inverse of ``split_run_state``: the two payloads as read back -> what ``LatteTrainer.load_training_state`` takes.
    base_model: with ``lora`` the frozen base's state dict, which the run directory does not hold."""
    if lora:
        return {**{k: v for k, v in state.items() if k not in ("rng", "lora_opt")}, "model": base_model,
                "lora": {"config": checkpoint["config"], "params": checkpoint["lora"], "ema": checkpoint["lora_ema"], **state["lora_opt"]}}
    return {**state, "model": checkpoint["model"], "ema": checkpoint["ema"]}


class RawClips:
    """Raw uint8 clips [T, Hs, Ws, 3] of any length and size, memory-mapped: per item the reference's temporal window, frame indices and
    flip coin (datasets/ucf101_datasets.py:198-216, video_transforms.py:386-427) from a generator seeded by (seed, step, micro, rank)."""
    frames = True
    accum = 1             # micro-batches per optimiser step (main sets it)

    def __init__(self, path, args, rank, world, seed):
        self.files = sorted(glob.glob(os.path.join(path, "*.npy")))
        if not self.files:
            raise SystemExit(f"no .npy clips under {path}")
        self.args, self.rank, self.world, self.seed = args, rank, world, seed
        self.num_frames = int(args.num_frames)

    def _clip(self, i):
        a = np.load(self.files[i], mmap_mode="r")             # mapped, not read: only the gathered frames are touched
        if a.dtype != np.uint8 or a.ndim != 4 or a.shape[-1] != 3:
            raise SystemExit(f"{self.files[i]}: raw clips are uint8 [T, Hs, Ws, 3], got {a.dtype} {a.shape}")
        return a

    def batch(self, step, n, micro=0):
        """-> ([(frames uint8 [num_frames, Hs, Ws, 3], flip)] * n, labels)"""
        import random
        from latte_amd import video_transforms
        s = data_seed(self.seed, step, micro, self.accum, self.rank, self.world)
        g = torch.Generator("cpu").manual_seed(s)
        transform, temporal_sample = video_transforms.get_transform(self.args, rng=random.Random(s))
        items, ys = [], []
        for i in torch.randint(0, len(self.files), (n,), generator=g).tolist():
            a = self._clip(i)
            start, end = temporal_sample(a.shape[0])
            assert end - start >= self.num_frames, f"{self.files[i]}: {a.shape[0]} frames, fewer than num_frames = {self.num_frames}"
            idx = video_transforms.frame_indices(start, end, self.num_frames)
            items.append((torch.from_numpy(np.ascontiguousarray(a[idx])), transform.draw_flips(1)[0]))
            ys.append(clip_label(self.files[i]))
        return items, torch.tensor(ys)


class MomentClips:
    """Stored VAE moments of raw clips (`moments_path`, a directory tools/encode_clips.py --moments wrote; latte_amd.MomentStore): the
    SAME draws as RawClips.batch for the same (seed, step, micro, rank) -- the clip index over the sorted file list, then per item the
    temporal window and the flip coin -- turned into rows of the store instead of gathered frames."""
    frames = False
    accum = 1             # micro-batches per optimiser step (main sets it)

    def __init__(self, store, args, rank, world, seed):
        self.store, self.args, self.rank, self.world, self.seed = store, args, rank, world, seed
        self.num_frames = int(args.num_frames)

    def batch(self, step, n, micro=0):
        """-> ([(clip, frame indices [num_frames], flip)] * n, labels)"""
        import random
        from latte_amd import video_transforms
        s = data_seed(self.seed, step, micro, self.accum, self.rank, self.world)
        g = torch.Generator("cpu").manual_seed(s)
        transform, temporal_sample = video_transforms.get_transform(self.args, rng=random.Random(s))
        frames, labels = self.store.clip_frames, self.store.labels
        items, ys = [], []
        for i in torch.randint(0, self.store.num_clips, (n,), generator=g).tolist():
            start, end = temporal_sample(frames[i])
            assert end - start >= self.num_frames, f"{self.store.names[i]}: {frames[i]} frames, fewer than num_frames = {self.num_frames}"
            items.append((i, video_transforms.frame_indices(start, end, self.num_frames), transform.draw_flips(1)[0]))
            ys.append(labels[i])
        return items, torch.tensor(ys)

    def latents(self, items, gen):
        """The items' latents [n, num_frames, 4, h, w] in one launch; the posterior noise is drawn item by item from ``gen``, as the
        raw path's per-item ``encode_video_raw`` draws it."""
        from latte_amd.vae import randn_tensor
        dev = torch.device("cuda", torch.cuda.current_device())
        noise = torch.cat([randn_tensor((self.num_frames, 4, *self.store.latent_hw), generator=gen, device=dev) for _ in items])
        x = self.store.sample_frames(np.concatenate([self.store.frame_rows(i, idx, fl) for i, idx, fl in items]), noise=noise)
        return x.view(len(items), self.num_frames, *x.shape[1:])


class MomentFrames:
    """The single images of joint training from stored moments (`frame_moments_path`: one-frame clips, plane 0): the indices
    ImageFrames.batch draws, as rows."""
    frames = False
    accum = 1

    def __init__(self, store, images, rank, world, seed):
        self.store, self.images, self.rank, self.world, self.seed = store, int(images), rank, world, seed

    def batch(self, step, n, micro=0):
        """-> (rows int64 [n * N], labels [n, N])"""
        g = torch.Generator("cpu").manual_seed(data_seed(self.seed, step, micro, self.accum, self.rank, self.world) + 500009)
        idx = draw_image_frames(self.store.num_clips, n, self.images, g).reshape(-1).tolist()
        labels = self.store.labels
        rows = np.concatenate([self.store.frame_rows(i, [0], False) for i in idx])
        return rows, torch.tensor([labels[i] for i in idx]).reshape(n, self.images)


class LatentClips:
    """Rank-sharded, seeded access to the latent clips (DistributedSampler(shuffle=True, seed=global_seed), train.py:136-151)."""
    accum = 1             # micro-batches per optimiser step (main sets it)

    def __init__(self, path, frames, latent, rank, world, seed, num_classes):
        self.synthetic = path in (None, "", "synthetic")
        self.shape = (frames, 4, latent, latent)
        self.rank, self.world, self.seed, self.num_classes = rank, world, seed, num_classes
        self.files = [] if self.synthetic else sorted(glob.glob(os.path.join(path, "*.npy")))
        if not self.synthetic and not self.files:
            raise SystemExit(f"no .npy latent clips under {path}")
        # uint8 frame clips [F, H, W, 3] at the training image size are encoded on the GPU per batch (frames=True)
        self.frames = False
        if self.files:
            first = np.load(self.files[0], mmap_mode="r")
            if first.dtype == np.uint8:
                self.shape = (frames, 8 * latent, 8 * latent, 3)
                self.frames = True

    def batch(self, step, n, micro=0):
        g = torch.Generator("cpu").manual_seed(data_seed(self.seed, step, micro, self.accum, self.rank, self.world))
        if self.synthetic:
            x = torch.randn(n, *self.shape, generator=g)
            y = torch.randint(0, max(self.num_classes, 1), (n,), generator=g)
            return x, y
        idx = torch.randint(0, len(self.files), (n,), generator=g).tolist()
        xs, ys = [], []
        for i in idx:
            a = np.load(self.files[i])
            assert a.shape == self.shape, f"{self.files[i]}: expected {self.shape}, got {a.shape}"
            xs.append(torch.from_numpy(a) if self.frames else torch.from_numpy(a).float())
            ys.append(clip_label(self.files[i]))
        return torch.stack(xs), torch.tensor(ys)


class ImageFrames:
    """The single frames of joint image-video training (`frame_data_path`, `use_image_num`): N per sample, drawn from the micro-batch's
    seeded generator (its seed offset keeps the draw apart from the clips')."""
    accum = 1             # micro-batches per optimiser step (main sets it)

    def __init__(self, path, images, latent, rank, world, seed, num_classes):
        self.synthetic = path in (None, "", "synthetic")
        self.images, self.latent = int(images), int(latent)
        self.rank, self.world, self.seed, self.num_classes = rank, world, seed, num_classes
        self.files = [] if self.synthetic else sorted(glob.glob(os.path.join(path, "*.npy")))
        if not self.synthetic and not self.files:
            raise SystemExit(f"no .npy frames under {path}")
        self.frames = bool(self.files) and np.load(self.files[0], mmap_mode="r").dtype == np.uint8
        self.shape = (8 * latent, 8 * latent, 3) if self.frames else (4, latent, latent)

    def batch(self, step, n, micro=0):
        """-> (x [n, N, 4, h, w] float latents or [n, N, H, W, 3] uint8 frames, labels [n, N])"""
        g = torch.Generator("cpu").manual_seed(data_seed(self.seed, step, micro, self.accum, self.rank, self.world) + 500009)
        if self.synthetic:
            x = torch.randn(n, self.images, *self.shape, generator=g)
            return x, torch.randint(0, max(self.num_classes, 1), (n, self.images), generator=g)
        idx = draw_image_frames(len(self.files), n, self.images, g)
        xs = []
        for i in idx.reshape(-1).tolist():
            a = np.load(self.files[i])
            assert a.shape == self.shape, f"{self.files[i]}: expected {self.shape}, got {a.shape}"
            xs.append(torch.from_numpy(a) if self.frames else torch.from_numpy(a).float())
        ys = torch.tensor([clip_label(self.files[i]) for i in idx.reshape(-1).tolist()]).reshape(n, self.images)
        return torch.stack(xs).reshape(n, self.images, *self.shape), ys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", required=True)
    ap.add_argument("--max-steps", type=int, default=None)
    ap.add_argument("--log-every", type=int, default=None)
    ap.add_argument("--ckpt-every", type=int, default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--moments-device", choices=("cuda", "cpu"), default="cuda",
                    help="where the stores of moments_path / frame_moments_path live: resident on the GPU, or in host memory (rows uploaded per batch)")
    a = ap.parse_args()
    args = latte_amd.load_config(a.config)
    rank, world, local = parallel.setup_distributed()
    assert torch.cuda.is_available(), "tools/train.py needs MI355X GPUs"
    device = torch.device("cuda", local)
    torch.cuda.set_device(device)
    accum = int(args.get("gradient_accumulation_steps") or 1)
    base_lr, warmup, lr_sched = float(args.learning_rate), int(args.get("lr_warmup_steps") or 0), str(args.get("lr_scheduler") or "constant")
    seed = int(args.global_seed)
    torch.manual_seed(seed)                                   # identical replicas (DDP broadcasts rank 0's weights, train.py:125)
    assert args.image_size % 8 == 0, "Image size must be divisible by 8 (for the VAE encoder)."   # train.py:88
    args.latent_size = args.image_size // 8
    nb = int(args.local_batch_size)
    args.max_batch = nb
    use_image_num = int(args.get("use_image_num") or 0)
    args.model = latte_preset_name(args.model)                # LatteIMG-* trains on the Latte-* preset of the same size
    model = latte_amd.get_models(args).to(device)
    if args.get("pretrained"):
        sd = latte_amd.find_model(args.pretrained)
        own = model.state_dict()
        model.load_state_dict({**own, **{k: v for k, v in sd.items() if k in own}})          # train.py:109-122
    diffusion = latte_amd.create_diffusion(timestep_respacing="")                                # train.py:92
    lora_rank = int(args.get("lora_rank") or 0)
    lora_kw = {}
    if lora_rank:
        if not args.get("pretrained"):
            raise SystemExit("lora_rank: LoRA fine-tunes a checkpoint -- set pretrained:")
        lora_kw = dict(lora_rank=lora_rank, lora_alpha=float(args.get("lora_alpha") or lora_rank),
                       lora_targets=args.get("lora_targets") or latte_amd.training.LORA_TARGETS)
    trainer = latte_amd.LatteTrainer(model, diffusion, max_batch=nb, lr=float(args.learning_rate), clip_max_norm=float(args.clip_max_norm),
                                     start_clip_iter=int(args.start_clip_iter), gradient_accumulation_steps=accum,
                                     use_image_num=use_image_num, **lora_kw)
    if lora_rank and rank == 0:
        print(f"LoRA: rank {lora_rank}, alpha {trainer.lora_alpha:g}, targets {','.join(trainer.lora_targets)}; "
              f"{trainer.lora_params.numel():,} trained parameters, the base is frozen", flush=True)
    # Replicas were initialised from the shared seed; from here every rank draws its own timesteps, noise and label-dropout
    # masks, as the reference does (train.py:62 `seed = args.global_seed + rank`): a global batch covers world * nb independent
    # draws, not nb draws replicated world times.
    torch.manual_seed(seed + rank)
    loss_fn = resolve_loss_fn(args.get("loss_fn"))
    if loss_fn is not None:
        if use_image_num:
            raise SystemExit("loss_fn: custom losses take video micro-batches only (no use_image_num)")
        if rank == 0:
            print(f"Custom loss: {args.get('loss_fn')} ({loss_fn.__module__}.{getattr(loss_fn, '__qualname__', loss_fn)})", flush=True)
    out_dir = a.out or args.results_dir
    first_step = 0
    if args.get("pretrained"):
        # train.py:195-196: the step counter continues from the checkpoint's file name (0100000.pt -> 100000), so gradient clipping
        # (start_clip_iter) and the checkpoint numbering carry on instead of restarting.  Only THAT counter: the checkpoint holds
        # model and ema, no optimiser state, so AdamW's moments start at zero and its bias correction at step 1 -- the engine
        # counts its applied updates itself (LatteTrainer docstring), as the reference's fresh torch.optim.AdamW does
        stem = os.path.basename(str(args.pretrained)).split(".")[0]
        if stem.isdigit():
            first_step = int(stem)
            trainer.train_steps = first_step
    if args.get("resume_from_checkpoint"):
        # train.py:176-192: the highest-numbered checkpoint of THIS run's results_dir -- with the state file beside it the whole run
        # comes back: parameters, EMA, AdamW moments, bias-correction count, loss scale and its growth count, step, random streams
        # (LoRA: the adapters, their EMA, their moments and the counters; the frozen base came from `pretrained:`)
        ck = (latest_lora_checkpoint if lora_rank else latest_checkpoint)(os.path.join(out_dir, "checkpoints"))
        if ck is None:
            if rank == 0:
                print(f"resume_from_checkpoint: no checkpoint under {out_dir}/checkpoints yet, starting a new run", flush=True)
        else:
            base_pt = ck[:-len(".lora.pt")] + ".pt" if lora_rank else ck          # the state files are named after <step>.pt
            if not os.path.isfile(state_path(base_pt)):
                raise SystemExit(f"resume_from_checkpoint: {ck} has no {os.path.basename(state_path(base_pt))} beside it"
                                 + ("" if lora_rank else " (written by an older version?); continue from its weights alone with `pretrained:`"))
            rest = torch.load(state_path(base_pt), map_location="cpu")
            trainer.load_training_state(join_run_state(torch.load(ck, map_location="cpu"), rest, lora_rank,
                                                       trainer.model_state_dict() if lora_rank else None))
            first_step = int(rest["train_steps"])
            if not lora_rank and checkpoint_step(ck) != first_step:
                raise SystemExit(f"resume_from_checkpoint: {ck} holds the state of step {first_step}")
            mine = rest if rank == 0 else (torch.load(state_path(base_pt, rank), map_location="cpu") if os.path.isfile(state_path(base_pt, rank)) else None)
            if mine is not None:
                set_rng_state(mine["rng"], device)
            sc = trainer.scaler_state()
            if rank == 0:
                print(f"Resumed from {ck}: step {first_step}" + ("" if lora_rank else f", loss scale {sc['loss_scale']:g}, applied updates "
                      f"{int(sc['applied_updates'])}, skipped updates {int(sc['skipped_updates'])}"), flush=True)
    moments = args.get("moments_path") not in (None, "")
    if moments and args.get("frame_interval") in (None, ""):
        raise SystemExit("moments_path: set frame_interval (the temporal window is drawn per item, as on raw clips)")
    raw = not moments and args.get("frame_interval") not in (None, "") and args.get("data_path") not in (None, "", "synthetic")
    if moments:                                               # stored moments of the raw clips: the raw path's draws, no encoder in the step
        data = MomentClips(latte_amd.MomentStore.load(args.moments_path, device=a.moments_device), args, rank, world, seed)
        if data.store.latent_hw != (args.latent_size, args.latent_size):
            raise SystemExit(f"moments_path holds {data.store.latent_hw} latents, image_size {args.image_size} needs {args.latent_size} x {args.latent_size}")
        if rank == 0:
            print(f"Moment store: {data.store.num_clips} clips, {sum(data.store.clip_frames)} frames x {len(data.store.planes)} planes, "
                  f"{data.store.dtype}, {data.store.nbytes / 2 ** 20:.1f} MiB on {a.moments_device}", flush=True)
    elif raw:                                                   # raw clips through the dataset's frame pipeline (datasets/__init__.py:13-76)
        from latte_amd import video_transforms
        data = RawClips(args.data_path, args, rank, world, seed)
        raw_transform, _ = video_transforms.get_transform(args)
    else:
        data = LatentClips(args.get("data_path"), int(args.num_frames), args.latent_size, rank, world, seed, int(args.get("num_classes") or 0))
    images = None
    if use_image_num:
        frame_path = "synthetic" if not moments and args.get("data_path") in (None, "", "synthetic") else args.get("frame_data_path")
        if args.get("frame_moments_path"):
            images = MomentFrames(latte_amd.MomentStore.load(args.frame_moments_path, device=a.moments_device), use_image_num, rank, world, seed)
        elif not frame_path:
            raise SystemExit("use_image_num: set frame_data_path (a directory of single frames) or frame_moments_path (their stored moments)")
        else:
            images = ImageFrames(frame_path, use_image_num, args.latent_size, rank, world, seed, int(args.get("num_classes") or 0))
        images.accum = accum
    vae = None
    if data.frames or (images is not None and images.frames):                                           # train.py:94 (+ the encoder): frames -> latents on the GPU every step
        if not args.get("pretrained_model_path"):
            raise SystemExit("data_path holds uint8 frame clips: set pretrained_model_path (its vae/ subfolder is the SD-VAE to encode with)")
        vae = latte_amd.AutoencoderKL.from_pretrained(args.pretrained_model_path, subfolder="vae", with_encoder=True).to(device)
    data.accum = accum
    max_steps = a.max_steps or int(args.max_train_steps)
    log_every = a.log_every or int(args.log_every)
    ckpt_every = a.ckpt_every or int(args.ckpt_every)
    if rank == 0:
        os.makedirs(os.path.join(out_dir, "checkpoints"), exist_ok=True)
        print(f"Model Parameters: {sum(p.numel() for p in model.parameters()):,}; world {world}, local batch {nb}")
    parallel.barrier()
    running, t0, log_steps = 0.0, time.time(), 0
    stuck_logs = 0      # consecutive log lines whose whole interval was skipped updates at the floor scale (or with scaling off)
    seen_skips = trainer.scaler_state()["skipped_updates"]
    for step in range(first_step + 1, max_steps + 1):
        trainer.lr = scheduled_lr(base_lr, step, warmup, lr_sched)     # get_scheduler(...).step(), train.py:169-173,233 (host side only)
        for micro in range(accum):                            # the optimiser step runs inside the last train_step of the window
            x, y = data.batch(step, nb, micro)
            stored = moments or isinstance(images, MomentFrames)
            if vae is not None or stored:                     # train.py:204-211, posterior noise from this micro-batch's seeded generator
                gen = torch.Generator(device).manual_seed(data_seed(seed, step, micro, accum, rank, world))
                if moments:                                   # the raw path's latents from the stored moments: one launch
                    x = data.latents(x, gen)
                elif raw:                                     # per item (sizes differ): one upload, one transform launch, the encode
                    x = torch.cat([vae.encode_video_raw(fr.to(device).unsqueeze(0), raw_transform, flip=[fl], generator=gen) for fr, fl in x])
                elif data.frames:
                    x = vae.encode_video_uint8(x.to(device), generator=gen)
            y_image = None
            if images is not None:                            # train_with_img.py:214-221: N single frames behind every clip
                xi, y_image = images.batch(step, nb, micro)
                if isinstance(images, MomentFrames):          # xi: rows of the image store
                    xi = images.store.sample_frames(xi, generator=gen).view(nb, use_image_num, 4, args.latent_size, args.latent_size)
                elif images.frames:
                    xi = vae.encode_video_uint8(xi.to(device), generator=gen)
                x = torch.cat([x.to(device).float(), xi.to(device).float()], dim=1)
                y_image = y_image.to(device) if int(args.extras) == 2 else None
            out = trainer.train_step(x.to(device), y=y.to(device) if int(args.extras) == 2 else None, y_image=y_image, loss_fn=loss_fn)
            running += float(out["loss"].mean()) / accum      # (the reference's loss.item(), train.py:239; undivided terms)
        log_steps += 1
        if step % log_every == 0:
            torch.cuda.synchronize()
            sps = log_steps / (time.time() - t0)
            avg = torch.tensor(running / log_steps, device=device)
            if world > 1:
                torch.distributed.all_reduce(avg)
                avg /= world
            # Overflow handling of the half-precision backward (LatteTrainer docstring): a non-finite gradient norm skips the update on
            # the device, silently.  The log line carries the counters, and a run that can no longer apply ANY update -- every step of
            # two log intervals skipped with the scale at its floor of 1 (or with dynamic scaling off) -- stops instead of burning its
            # budget on zero updates (a diverged model or an f16 forward overflow no loss scale cures).
            sc = trainer.scaler_state()
            new_skips = sc["skipped_updates"] - seen_skips
            seen_skips = sc["skipped_updates"]
            stuck = new_skips >= log_steps and (sc["loss_scale"] <= 1.0 or not sc["dynamic"])
            stuck_logs = stuck_logs + 1 if stuck else 0
            if rank == 0:
                print(f"(step={step:07d}) Train Loss: {float(avg):.4f}, Gradient Norm: {float(out['grad_norm']):.4f}, "
                      f"Train Steps/Sec: {sps:.2f}, samples/s: {sps * nb * accum * world:.1f}, loss scale: {sc['loss_scale']:g}, "
                      f"skipped updates: {int(sc['skipped_updates'])} (+{int(new_skips)})", flush=True)
                if new_skips and not stuck:
                    print(f"  warning: {int(new_skips)} of the last {log_steps} updates were skipped (non-finite gradient norm)", flush=True)
            if stuck_logs >= 2:
                raise RuntimeError(f"training is stuck: every update of the last {2 * log_steps} steps was skipped (non-finite gradient norm) "
                                   f"with the loss scale at {sc['loss_scale']:g}" + ("" if sc["dynamic"] else " and dynamic scaling off")
                                   + " -- the model has diverged or an f16 activation overflows; lower the learning rate or train with compute_dtype='bf16'")
            running, t0, log_steps = 0.0, time.time(), 0
        if step % ckpt_every == 0 or step == max_steps:
            # <step>.pt stays the reference's two entries; the rest of the run goes beside it (read back by resume_from_checkpoint):
            # every rank its random state, rank 0 also the AdamW moments and the counters
            path = os.path.join(out_dir, "checkpoints", f"{step:07d}.pt")
            mine = {"rng": rng_state(device), "train_steps": step}
            if rank == 0:
                suffix, payload, rest = split_run_state(trainer.training_state(), lora_rank)
                torch.save(payload, path[:-len(".pt")] + suffix)
                print(f"Saved checkpoint to {path[:-len('.pt')] + suffix}", flush=True)
                mine.update(rest)
            torch.save(mine, state_path(path, rank))
            parallel.barrier()
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
