"""Encode a directory of uint8 frame clips into the latent clips tools/train.py reads, once instead of every epoch.

  python tools/encode_clips.py --vae <pretrained_model_path>/vae --src <frame clips> --dst <latent clips> [--seed 0]

In: .npy uint8 [F, H, W, 3] per clip (H == W, a multiple of 128).  Out: .npy fp32 [F, 4, H/8, W/8] under the SAME file name (the
class-label prefix `<label>_...` tools/train.py parses survives) = vae.encode(x).latent_dist.sample().mul_(0.18215) of the reference's
train.py:204-211, computed by AutoencoderKL.encode_video_uint8 on the MI355X with posterior noise from a generator seeded by --seed.

  python tools/encode_clips.py --moments --config <train yaml> --vae <...>/vae --src <RAW clips> --dst <moment files> [--dtype f16|fp32]

--moments: in, RAW uint8 clips .npy [T, Hs, Ws, 3] of any length and size; out, per clip .npy [T, P, 8, h, w] under the same name --
the posterior moments (mean | logvar) of EVERY frame through the config's data-set transform (`dataset`, `image_size`), under each
flip plane (P = 2, or 1 for a pipeline without a flip): what tools/train.py reads as `moments_path` (latte_amd.MomentStore).  No noise
is drawn: window, flip and posterior sample are redrawn every training step.
"""
import argparse
import glob
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import latte_amd  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--vae", required=True, help="diffusers AutoencoderKL directory (config.json + diffusion_pytorch_model.*)")
    ap.add_argument("--src", required=True, help="directory of uint8 frame clips .npy [F, H, W, 3]")
    ap.add_argument("--dst", required=True, help="output directory of latent clips .npy [F, 4, H/8, W/8]")
    ap.add_argument("--seed", type=int, default=0, help="seed of the posterior noise")
    ap.add_argument("--max-frames", type=int, default=16, help="frames per engine call")
    ap.add_argument("--moments", action="store_true", help="write the posterior moments of every frame of RAW clips (see above), not sampled latents")
    ap.add_argument("--config", default=None, help="--moments: the training YAML whose dataset / image_size select the frame transform")
    ap.add_argument("--dtype", choices=("f16", "fp32"), default="f16", help="--moments: storage type of the moment files")
    a = ap.parse_args()
    if a.moments and not a.config:
        ap.error("--moments needs --config (the training YAML)")
    files = sorted(glob.glob(os.path.join(a.src, "*.npy")))
    if not files:
        raise SystemExit(f"no .npy frame clips under {a.src}")
    assert torch.cuda.is_available(), "tools/encode_clips.py needs an MI355X"
    device = torch.device("cuda", torch.cuda.current_device())
    vae = latte_amd.AutoencoderKL.from_pretrained(a.vae, with_encoder=True, max_frames=a.max_frames).to(device)
    gen = torch.Generator(device).manual_seed(a.seed)
    os.makedirs(a.dst, exist_ok=True)
    if a.moments:
        from latte_amd import video_transforms
        args = latte_amd.load_config(a.config)
        if args.get("frame_interval") in (None, ""):
            args.frame_interval = 1                               # (the temporal crop is not used here)
        transform, _ = video_transforms.get_transform(args)
        for f in files:                                           # one clip at a time: the raw frames are mapped, never all in memory
            name = os.path.splitext(os.path.basename(f))[0]
            store = latte_amd.MomentStore.build(vae, [(name, np.load(f, mmap_mode="r"))], transform, dtype=a.dtype)
            store.save(a.dst)
            print(f"{name}: {store.clip_frames[0]} frames x {len(store.planes)} planes -> {store.dtype} {store.nbytes / 2 ** 20:.2f} MiB", flush=True)
        return
    for f in files:
        clip = np.load(f)
        if clip.dtype != np.uint8 or clip.ndim != 4 or clip.shape[-1] != 3:
            raise SystemExit(f"{f}: expected uint8 [F, H, W, 3], got {clip.dtype} {clip.shape}")
        lat = vae.encode_video_uint8(torch.from_numpy(clip)[None].to(device), generator=gen)[0]
        np.save(os.path.join(a.dst, os.path.basename(f)), lat.cpu().numpy())
        print(f"{os.path.basename(f)}: {tuple(clip.shape)} -> {tuple(lat.shape)}", flush=True)


if __name__ == "__main__":
    main()
