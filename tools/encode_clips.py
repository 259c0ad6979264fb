"""Encode a directory of uint8 frame clips into the latent clips tools/train.py reads, once instead of every epoch.

  python tools/encode_clips.py --vae <pretrained_model_path>/vae --src <frame clips> --dst <latent clips> [--seed 0]

In: .npy uint8 [F, H, W, 3] per clip (H == W, a multiple of 128).  Out: .npy fp32 [F, 4, H/8, W/8] under the SAME file name (the
class-label prefix `<label>_...` tools/train.py parses survives) = vae.encode(x).latent_dist.sample().mul_(0.18215) of the reference's
train.py:204-211, computed by AutoencoderKL.encode_video_uint8 on the MI355X with posterior noise from a generator seeded by --seed.
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
    a = ap.parse_args()
    files = sorted(glob.glob(os.path.join(a.src, "*.npy")))
    if not files:
        raise SystemExit(f"no .npy frame clips under {a.src}")
    assert torch.cuda.is_available(), "tools/encode_clips.py needs an MI355X"
    device = torch.device("cuda", torch.cuda.current_device())
    vae = latte_amd.AutoencoderKL.from_pretrained(a.vae, with_encoder=True, max_frames=a.max_frames).to(device)
    gen = torch.Generator(device).manual_seed(a.seed)
    os.makedirs(a.dst, exist_ok=True)
    for f in files:
        clip = np.load(f)
        if clip.dtype != np.uint8 or clip.ndim != 4 or clip.shape[-1] != 3:
            raise SystemExit(f"{f}: expected uint8 [F, H, W, 3], got {clip.dtype} {clip.shape}")
        lat = vae.encode_video_uint8(torch.from_numpy(clip)[None].to(device), generator=gen)[0]
        np.save(os.path.join(a.dst, os.path.basename(f)), lat.cpu().numpy())
        print(f"{os.path.basename(f)}: {tuple(clip.shape)} -> {tuple(lat.shape)}", flush=True)


if __name__ == "__main__":
    main()
