"""Side measurement: the SD-VAE ENCODER (AutoencoderKL.encode, the reference's training-step call train.py:204-211) on one
16-frame 256x256 clip, random sd-vae-shaped weights.  Prints ONE JSON line: ms per clip for the uint8-frames path of
AutoencoderKL.encode_video_uint8 (normalise, encode, posterior sample, scale), the per-class table of latte_vae_profile_encode, the
algorithmic work counted from the layer shapes, and the convolution class's rate.

  python tools/vae_encode_bench.py [--frames 16] [--size 256] [--reps 5]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import latte_amd  # noqa: E402
from latte_amd.random_init import vae_encoder_state_dict  # noqa: E402


def encoder_flops(size, block_out=(128, 256, 512, 512), layers=2):
    """Multiply-adds x 2 per frame, by kernel class: conv3x3 (the implicit-GEMM convolutions incl. the down-samplers),
    attention_and_1x1 (mid-block attention + the 1x1 shortcuts), small (conv_in, conv_out + quant_conv)."""
    f = {"conv3x3": 0, "attention_and_1x1": 0, "small": 0}
    r, prev = size, block_out[0]
    f["small"] += 2 * r * r * block_out[0] * 3 * 9
    for i, c in enumerate(block_out):
        for k in range(layers):
            cin = prev if k == 0 else c
            f["conv3x3"] += 2 * r * r * 9 * (cin * c + c * c)
            if cin != c:
                f["attention_and_1x1"] += 2 * r * r * cin * c
        prev = c
        if i != len(block_out) - 1:
            r //= 2
            f["conv3x3"] += 2 * r * r * 9 * c * c
    top, L = block_out[-1], r * r
    f["conv3x3"] += 2 * 2 * L * 9 * top * top                                # mid-block resnets
    f["attention_and_1x1"] += 4 * 2 * L * top * top + 2 * 2 * L * L * top    # q, k, v, out projections; q k^T and P v
    f["small"] += 2 * L * 8 * top * 9 + 2 * L * 8 * 8
    return f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda")
    vae = latte_amd.AutoencoderKL(max_frames=a.frames, with_encoder=True)
    vae.load_state_dict(vae_encoder_state_dict(0))
    vae.to(dev)
    g = torch.Generator("cpu").manual_seed(5000)
    frames = torch.randint(0, 256, (1, a.frames, a.size, a.size, 3), generator=g, dtype=torch.uint8).to(dev)
    gen = torch.Generator(dev).manual_seed(0)
    vae.encode_video_uint8(frames, generator=gen)            # warm-up (handle, weights)
    torch.cuda.synchronize()
    times = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        vae.encode_video_uint8(frames, generator=gen)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    prof = vae.profile_encode(frames[0].contiguous(), in_mode=1)
    fl = encoder_flops(a.size)
    total = sum(fl.values()) * a.frames
    conv_ms = prof["conv3x3"][0]
    print(json.dumps({
        "metric": "vae_encode_ms_per_clip", "frames": a.frames, "size": a.size,
        "ms_per_clip_median": round(sorted(times)[len(times) // 2], 3), "ms_all": [round(t, 3) for t in times],
        "tflop_per_clip": round(total / 1e12, 4), "tflop_per_frame": round(total / a.frames / 1e12, 5),
        "classes_ms_launches": {k: [round(v[0], 3), v[1]] for k, v in prof.items()},
        "conv3x3_tflops_per_s": round(fl["conv3x3"] * a.frames / (conv_ms * 1e-3) / 1e12, 1) if conv_ms > 0 else None,
    }))


if __name__ == "__main__":
    main()
