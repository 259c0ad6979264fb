"""sample/sample_t2x.py of the reference on the MI355X engine: Latte-1 text-to-video.

  python tools/sample_t2x.py --config configs/t2v_sample.yaml [--random] [--steps N] [--layers L] [--sample-method NAME]
                             [--video-length L --window-stride S]

--video-length L above the config's ``video_length`` (the transformer's clip length) with --window-stride S samples the longer clip by
overlapping temporal windows (LattePipeline(window_stride=), not in the reference); the VAE decodes all L frames.

With a real checkpoint directory (`pretrained_model_path` holding transformer/, vae/, tokenizer/, text_encoder/) the flow is
the reference's (sample_t2x.py:21-140): the T5 tokenizer from `transformers`, the T5 encoder on the engine
(`latte_amd.T5EncoderModel.from_pretrained`), `LatteT2V.from_pretrained_2d`, `AutoencoderKL.from_pretrained`, a DDIM scheduler,
`LattePipeline(...)`, one video per prompt.  Offline there are no weights: `--random` builds randomly initialised models, the text
encoder among them (`--t5-layers` of the XXL shape), and a deterministic stand-in tokenizer (`latte_amd.t5.HashTokenizer`), so the
run goes prompt string -> ids -> T5 -> denoiser -> VAE -> mp4 on the device path and times it.  Videos are written as .mp4
(Motion-JPEG samples, latte_amd.video_io).  `sample_method` picks one of the five self-contained schedulers of latte_amd/schedulers.py
(DDIM, EulerDiscrete, EulerAncestralDiscrete, HeunDiscrete, DPMSolverMultistep), each of which runs its whole guided chain inside the
engine; the reference's other five names are refused (INTEGRATION.md says why), and any diffusers scheduler object can be passed to
LattePipeline instead.
"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import latte_amd  # noqa: E402
from latte_amd import schedulers  # noqa: E402

# sample_t2x.py:43-114: sample_method -> scheduler class
SAMPLE_METHODS = {
    "DDIM": schedulers.DDIMScheduler,
    "EulerDiscrete": schedulers.EulerDiscreteScheduler,
    "EulerAncestralDiscrete": schedulers.EulerAncestralDiscreteScheduler,
    "HeunDiscrete": schedulers.HeunDiscreteScheduler,
    "DPMSolverMultistep": schedulers.DPMSolverMultistepScheduler,
}
REFUSED_METHODS = ("DDPM", "PNDM", "DPMSolverSinglestep", "DEISMultistep", "KDPM2AncestralDiscrete")


def make_scheduler(args):
    name = args.sample_method
    if name not in SAMPLE_METHODS:
        known = "one of the reference's methods without an offline stand-in" if name in REFUSED_METHODS else "not a sample_method"
        raise SystemExit(f"sample_method {name!r} is {known}; the methods that run are {', '.join(SAMPLE_METHODS)} "
                         "(or pass a diffusers scheduler object to LattePipeline)")
    kw = dict(beta_start=args.beta_start, beta_end=args.beta_end, beta_schedule=args.beta_schedule)
    if name == "DDIM":
        kw["clip_sample"] = False
    return SAMPLE_METHODS[name](**kw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", required=True)
    ap.add_argument("--random", action="store_true", help="random weights and a stand-in tokenizer (no checkpoints offline)")
    ap.add_argument("--t5-layers", type=int, default=24, help="--random: depth of the randomly initialised T5 encoder (XXL shape)")
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--sample-method", default=None, help="overrides the config's sample_method: " + ", ".join(SAMPLE_METHODS))
    ap.add_argument("--layers", type=int, default=28)
    ap.add_argument("--out", default=None)
    ap.add_argument("--video-length", type=int, default=0, help="frames to sample, >= the config's video_length: a longer clip by temporal windows")
    ap.add_argument("--window-stride", type=int, default=0, help="frames between window starts, 1 ... video_length (default video_length // 2)")
    a = ap.parse_args()
    args = latte_amd.load_config(a.config)
    if a.sample_method:
        args.sample_method = a.sample_method
    torch.set_grad_enabled(False)
    assert torch.cuda.is_available(), "sample_t2x needs an MI355X"
    device = "cuda"
    cdt = "f16"                       # sample_t2x.py:29 .to(device, dtype=torch.float16): the only operand type of latte_amd.LatteT2V
    latent = args.image_size[0] // 8
    scheduler = make_scheduler(args)
    total = a.video_length or args.video_length                # frames sampled and decoded; the transformer stays at args.video_length
    stride = (a.window_stride or max(1, args.video_length // 2)) if (a.video_length or a.window_stride) else None
    pair = 2 * (len(latte_amd.window_starts(total, args.video_length, stride)) if stride else 1)   # the guidance pair's clips per step
    tokenizer = text_encoder = None
    if a.random:
        from latte_amd.random_init import t2v_state_dict, t5_state_dict, vae_decoder_state_dict
        from latte_amd.t5 import HashTokenizer
        tokenizer = HashTokenizer()
        text_encoder = latte_amd.T5EncoderModel(num_layers=a.t5_layers, max_batch=1).load_state_dict(t5_state_dict(0, num_layers=a.t5_layers))
        transformer = latte_amd.LatteT2V(num_layers=a.layers, sample_size=latent, video_length=args.video_length,
                                         compute_dtype=cdt, max_batch=pair).load_state_dict(t2v_state_dict(0, num_layers=a.layers))
        if args.enable_vae_temporal_decoder:                       # sample_t2x.py:31-32
            from latte_amd.random_init import vae_temporal_decoder_state_dict
            vae = latte_amd.AutoencoderKLTemporalDecoder(latent_size=latent, max_frames=14, compute_dtype="f16")
            vae.load_state_dict(vae_temporal_decoder_state_dict(0))
        else:
            vae = latte_amd.AutoencoderKL(latent_size=latent, max_frames=total, compute_dtype="f16")
            vae.load_state_dict(vae_decoder_state_dict(0))
    else:
        from transformers import T5Tokenizer
        p = args.pretrained_model_path
        transformer = latte_amd.LatteT2V.from_pretrained_2d(p, subfolder="transformer", video_length=args.video_length,
                                                            compute_dtype=cdt, max_batch=pair)
        if args.enable_vae_temporal_decoder:                       # sample_t2x.py:31-32
            vae = latte_amd.AutoencoderKLTemporalDecoder.from_pretrained(p, subfolder="vae_temporal_decoder", latent_size=latent,
                                                                         max_frames=14)
        else:
            vae = latte_amd.AutoencoderKL.from_pretrained(p, subfolder="vae", latent_size=latent, max_frames=total)
        tokenizer = T5Tokenizer.from_pretrained(p, subfolder="tokenizer")
        text_encoder = latte_amd.T5EncoderModel.from_pretrained(p, subfolder="text_encoder", max_batch=1).eval()
    pipe = latte_amd.LattePipeline(vae=vae, text_encoder=text_encoder, tokenizer=tokenizer, scheduler=scheduler,
                                   transformer=transformer).to(device)
    out_dir = a.out or args.save_img_path
    os.makedirs(out_dir, exist_ok=True)
    steps = a.steps or args.num_sampling_steps
    g = torch.Generator("cpu").manual_seed(int(args.seed or 0))
    for n, prompt in enumerate(args.text_prompt):
        print(f"Processing the ({prompt}) prompt")
        kw = dict(prompt=prompt)
        torch.cuda.synchronize()
        t0 = time.time()
        video = pipe(video_length=total, window_stride=stride, height=args.image_size[0], width=args.image_size[1],
                     num_inference_steps=steps, guidance_scale=args.guidance_scale,
                     enable_temporal_attentions=args.enable_temporal_attentions, num_images_per_prompt=1, mask_feature=True,
                     enable_vae_temporal_decoder=bool(args.enable_vae_temporal_decoder), generator=g, **kw).video
        torch.cuda.synchronize()
        dt = time.time() - t0
        path = os.path.join(out_dir, f"{n:03d}.mp4")
        latte_amd.write_mp4(path, video[0], fps=8)                    # sample_t2x.py:137 imageio.mimwrite(..., fps=8)
        print(f"  {steps} steps + decode in {dt:.2f} s ({steps / dt:.2f} steps/s incl. decode) -> {path} {tuple(video.shape)}")


if __name__ == "__main__":
    main()
