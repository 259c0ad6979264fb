"""Edit a real clip by DDIM inversion: invert its latent under its own label, regenerate it under another one.

  python tools/invert.py --config configs/tiny_sample.yaml (--ckpt model.pt | --random) --data DIR|synthetic
                         [--label K] [--target-label K] [--steps 50] [--cfg-scale 1.0] [--out DIR] [--max-clips N] [--vae DIR]

The model comes from a sample YAML exactly as tools/sample.py builds it; --random re-draws the zero-initialised adaLN / final layers
instead of loading a checkpoint, so the whole device path runs without weights (plumbing, not a picture worth looking at).  --data is
a directory of latent clips (.npy [F, 4, h, w], already scaled by 0.18215, as tools/encode_clips.py writes them; source label = file-
name prefix unless --label is given) or "synthetic".

Per clip: ``ddim_reverse_sample_loop`` over the respaced indices 0 ... T-2 under the source label -- ONE latte_invert_loop call -- which
ends at level T-1, exactly where ``ddim_sample_loop`` takes its input (level T would be pure noise, one step further); then
``ddim_sample_loop`` from that latent under the target label.  --cfg-scale above 1 drives ``forward_with_cfg`` on the doubled batch
[label, null] in both directions.  clip_denoised is off in both, as tools/sample.py samples.  The regenerated latents are decoded with
AutoencoderKL (``pretrained_model_path`` of the YAML or --vae; a randomly initialised decoder otherwise) and written as .mp4.

Prints one JSON line per clip; where the target label is the source label, "reconstruction_mse" is the latent-space mean squared
difference between the clip and its round trip.  It is small only for a trained model at cfg-scale 1: the round trip of an untrained
model does not come back."""
import argparse
import glob
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import latte_amd  # noqa: E402
from latte_amd import create_diffusion, find_model, get_models  # noqa: E402


def clip_label(path):
    name = os.path.basename(path)
    return int(name.split("_")[0]) if name.split("_")[0].isdigit() else 0


def clips(cli, args):
    """-> iterator of (name, x0 [F, 4, h, w] float32, source label)"""
    shape = (args.num_frames, 4, args.latent_size, args.latent_size)
    if cli.data == "synthetic":
        g = torch.Generator("cpu").manual_seed(int(args.get("seed") or 0))
        for k in range(cli.max_clips or 2):
            yield f"synthetic_{k}", torch.randn(*shape, generator=g).clamp(-1.0, 1.0), int(torch.randint(0, max(int(args.num_classes), 1), (1,), generator=g))
        return
    files = sorted(glob.glob(os.path.join(cli.data, "*.npy")))
    if not files:
        raise SystemExit(f"no .npy latent clips under {cli.data}")
    for f in files[:cli.max_clips or None]:
        a = np.load(f)
        if a.dtype == np.uint8 or tuple(a.shape[1:]) != shape[1:] or a.shape[0] < shape[0]:
            raise SystemExit(f"{f}: expected a latent clip [F >= {shape[0]}, 4, {shape[2]}, {shape[3]}] (tools/encode_clips.py), "
                             f"got {a.dtype} {tuple(a.shape)}")
        yield os.path.splitext(os.path.basename(f))[0], torch.from_numpy(np.ascontiguousarray(a[:shape[0]], dtype=np.float32)), clip_label(f)


def main(args, cli):
    torch.set_grad_enabled(False)
    if not torch.cuda.is_available():
        raise SystemExit("tools/invert.py needs an MI355X (latte_amd has no CPU fallback)")
    device = "cuda"
    guided = cli.cfg_scale > 1.0
    args.latent_size = args.image_size // 8
    args.max_batch = 2 if guided else 1
    model = get_models(args).to(device)
    if cli.ckpt:
        model.load_state_dict(find_model(cli.ckpt))
    else:
        g = torch.Generator("cpu").manual_seed(1)
        for _, p in model.named_parameters():
            if p.requires_grad and float(p.detach().abs().max()) == 0.0:
                p.copy_(torch.randn(p.shape, generator=g) * 0.02)
        model.mark_weights_dirty()
    model.eval()
    diffusion = create_diffusion(str(cli.steps), learn_sigma=bool(args.learn_sigma))
    T = diffusion.num_timesteps
    if cli.vae or args.get("pretrained_model_path") and os.path.isdir(os.path.join(args.pretrained_model_path, "vae")):
        root = cli.vae or os.path.join(args.pretrained_model_path, "vae")
        vae = latte_amd.AutoencoderKL.from_pretrained(root, latent_size=args.latent_size, max_frames=args.num_frames).to(device)
    else:
        from latte_amd.random_init import vae_decoder_state_dict
        vae = latte_amd.AutoencoderKL(latent_size=args.latent_size, max_frames=args.num_frames)
        vae.load_state_dict(vae_decoder_state_dict(0))
        vae.to(device)
    if args.get("use_fp16"):
        model.to(dtype=torch.float16)
        vae.to(dtype=torch.float16)
    fn = model.forward_with_cfg if guided else model.forward
    conditional = int(args.extras) == 2

    def kwargs(label):
        kw = dict(use_fp16=bool(args.get("use_fp16")))
        if conditional:
            y = torch.tensor([label], device=device)
            kw["y"] = torch.cat([y, torch.full_like(y, int(args.num_classes))]) if guided else y
        if guided:
            kw["cfg_scale"] = cli.cfg_scale
        return kw

    os.makedirs(cli.out, exist_ok=True)
    results = []
    for name, x0, src in clips(cli, args):
        src = cli.label if cli.label is not None else src
        dst = cli.target_label if cli.target_label is not None else src
        x = x0.unsqueeze(0).to(device)
        if guided:
            x = torch.cat([x, x], 0)
        inverted = diffusion.ddim_reverse_sample_loop(fn, x, clip_denoised=False, model_kwargs=kwargs(src), end_index=T - 2)
        regen = diffusion.ddim_sample_loop(fn, inverted.shape, inverted, clip_denoised=False, model_kwargs=kwargs(dst), device=device)
        regen = regen[:1]
        f, c, h, w = regen.shape[1:]
        frames = vae.decode(regen.reshape(f, c, h, w) / 0.18215).sample
        video = ((frames * 0.5 + 0.5) * 255).add_(0.5).clamp_(0, 255).to(dtype=torch.uint8).cpu().permute(0, 2, 3, 1).contiguous()
        path = os.path.join(cli.out, f"{name}_label{src}_to_{dst}.mp4")
        latte_amd.write_mp4(path, video, fps=8)
        rec = {"clip": name, "label": src, "target_label": dst, "steps": T, "cfg_scale": cli.cfg_scale, "video": path,
               "inverted_std": float(inverted[:1].std())}
        if dst == src:
            rec["reconstruction_mse"] = float(((regen - x[:1]) ** 2).mean())
        print(json.dumps(rec), flush=True)
        results.append(rec)
    return results


def parse(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument("--config", type=str, default=os.path.join(ROOT, "configs", "tiny_sample.yaml"))
    parser.add_argument("--ckpt", type=str, default="")
    parser.add_argument("--random", action="store_true", help="run without weights: re-draw the zero-initialised layers")
    parser.add_argument("--data", type=str, required=True, help='directory of latent clips .npy [F, 4, h, w], or "synthetic"')
    parser.add_argument("--label", type=int, default=None, help="source label (default: the file-name prefix)")
    parser.add_argument("--target-label", type=int, default=None, help="label to regenerate under (default: the source label)")
    parser.add_argument("--steps", type=int, default=50)
    parser.add_argument("--cfg-scale", type=float, default=1.0)
    parser.add_argument("--out", type=str, default="./sample_videos")
    parser.add_argument("--max-clips", type=int, default=0)
    parser.add_argument("--vae", type=str, default="")
    cli = parser.parse_args(argv)
    if bool(cli.ckpt) == bool(cli.random):
        parser.error("give exactly one of --ckpt FILE and --random")
    if cli.steps < 2:
        parser.error("--steps must be at least 2 (the inversion runs indices 0 ... steps-2)")
    if cli.data != "synthetic" and not os.path.isdir(cli.data):
        parser.error(f'--data must be a directory of latent clips or "synthetic", got {cli.data!r}')
    conf = latte_amd.load_config(cli.config)
    for k, v in (("--label", cli.label), ("--target-label", cli.target_label)):
        if v is not None and not 0 <= v < int(conf.num_classes):
            parser.error(f"{k} must be in [0, {int(conf.num_classes)})")
    return conf, cli


if __name__ == "__main__":
    main(*parse())
