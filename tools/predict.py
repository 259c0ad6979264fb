"""Hold part of a real clip fixed and generate the rest: animate a first frame, continue a clip, fill between key frames, repaint a region.

  python tools/predict.py --config configs/tiny_sample.yaml (--ckpt model.pt | --random) --data DIR|synthetic
                          --task prefix:K | keyframes:i,j,... | box:y0,x0,y1,x1
                          [--method ddim|ddpm] [--resample R] [--steps 50] [--label K] [--cfg-scale 1.0] [--out DIR] [--max-clips N]
                          [--vae DIR] [--seed 0]

The model comes from a sample YAML exactly as tools/sample.py builds it; --random re-draws the zero-initialised adaLN / final layers
instead of loading a checkpoint, so the whole device path runs without weights (plumbing, not a picture worth looking at).  --data is
a directory of uint8 frame clips (.npy [F, H, W, 3], H == W == image_size of the YAML, as tools/encode_clips.py reads them; label =
file-name prefix unless --label is given) or "synthetic".

Per clip: the frames are encoded by the VAE encoder (``AutoencoderKL.encode_video_uint8``), the mask is built by ``latte_amd.known_mask``
-- prefix:K = the first K frames known, keyframes = the listed frames, box = the latent-pixel box [y0, y1) x [x0, x1) of every frame --
and ``SpacedDiffusion.known_sample_loop`` generates the rest: ONE latte_sample_loop_known call per chain segment, the known part of
the latents overwritten after every step with the clip diffused to the level just reached, every step repeated --resample times.
--cfg-scale above 1 drives ``forward_with_cfg`` on the doubled batch [label, null].  The result is decoded and written as .mp4 with the
input, the mask and the result side by side.  With --vae (or ``pretrained_model_path`` of the YAML) the VAE is loaded; a randomly
initialised one otherwise.

Prints one JSON line per clip.  "known_max_abs_diff" is the difference between the result's known latents and the clip's: 0 by
construction.  Nothing is claimed about the quality of the generated part: there is no trained checkpoint in this repository."""
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


def parse_task(task, frames, latent):
    """-> keyword arguments of latte_amd.known_mask."""
    kind, _, val = task.partition(":")
    try:
        nums = [int(v) for v in val.split(",")] if val else []
    except ValueError:
        nums = None
    if kind == "prefix" and nums and len(nums) == 1 and 1 <= nums[0] < frames:
        return dict(frames=list(range(nums[0])))
    if kind == "keyframes" and nums and all(-frames <= v < frames for v in nums):
        return dict(frames=nums)
    if kind == "box" and nums and len(nums) == 4 and 0 <= nums[0] < nums[2] <= latent and 0 <= nums[1] < nums[3] <= latent:
        return dict(box=tuple(nums))
    raise SystemExit(f"--task {task!r}: prefix:K (1 <= K < {frames}), keyframes:i,j,... (frame indices) or box:y0,x0,y1,x1 "
                     f"(latent pixels, within {latent} x {latent})")


def clips(cli, args):
    """-> iterator of (name, frames uint8 [F, S, S, 3], label)"""
    F, S = int(args.num_frames), int(args.image_size)
    if cli.data == "synthetic":
        g = torch.Generator("cpu").manual_seed(cli.seed)
        yy, xx = torch.meshgrid(torch.arange(S), torch.arange(S), indexing="ij")
        for k in range(cli.max_clips or 2):
            # a bright square drifting over a gradient: something to look at in the side-by-side video
            base = ((xx + yy).float() / (2 * S - 2) * 160).to(torch.uint8)[None, :, :, None].repeat(F, 1, 1, 3)
            y0, x0 = (int(v) for v in torch.randint(0, S // 2, (2,), generator=g))
            for f in range(F):
                base[f, y0:y0 + S // 4, x0 + f * (S // (4 * F)):x0 + f * (S // (4 * F)) + S // 4] = 240
            yield f"synthetic_{k}", base, int(torch.randint(0, max(int(args.num_classes), 1), (1,), generator=g))
        return
    files = sorted(glob.glob(os.path.join(cli.data, "*.npy")))
    if not files:
        raise SystemExit(f"no .npy frame clips under {cli.data}")
    for f in files[:cli.max_clips or None]:
        a = np.load(f)
        if a.dtype != np.uint8 or a.ndim != 4 or tuple(a.shape[1:]) != (S, S, 3) or a.shape[0] < F:
            raise SystemExit(f"{f}: expected uint8 frames [F >= {F}, {S}, {S}, 3], got {a.dtype} {tuple(a.shape)}")
        yield os.path.splitext(os.path.basename(f))[0], torch.from_numpy(np.ascontiguousarray(a[:F])), clip_label(f)


def main(args, cli):
    torch.set_grad_enabled(False)
    if not torch.cuda.is_available():
        raise SystemExit("tools/predict.py needs an MI355X (latte_amd has no CPU fallback)")
    device = "cuda"
    guided = cli.cfg_scale > 1.0
    args.latent_size = args.image_size // 8
    args.max_batch = 2 if guided else 1
    F, L = int(args.num_frames), int(args.latent_size)
    mask_kw = parse_task(cli.task, F, L)
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
    if cli.vae or args.get("pretrained_model_path") and os.path.isdir(os.path.join(args.pretrained_model_path, "vae")):
        root = cli.vae or os.path.join(args.pretrained_model_path, "vae")
        vae = latte_amd.AutoencoderKL.from_pretrained(root, latent_size=L, max_frames=F, with_encoder=True).to(device)
    else:
        from latte_amd.random_init import vae_decoder_state_dict, vae_encoder_state_dict
        vae = latte_amd.AutoencoderKL(latent_size=L, max_frames=F, with_encoder=True)
        vae.load_state_dict({**vae_decoder_state_dict(0), **vae_encoder_state_dict(0)})
        vae.to(device)
    if args.get("use_fp16"):
        model.to(dtype=torch.float16)
    fn = model.forward_with_cfg if guided else model.forward
    conditional = int(args.extras) == 2
    gen = torch.Generator(device).manual_seed(cli.seed)
    torch.manual_seed(cli.seed)
    os.makedirs(cli.out, exist_ok=True)
    results = []
    for name, frames, label in clips(cli, args):
        label = cli.label if cli.label is not None else label
        known = vae.encode_video_uint8(frames[None].to(device), generator=gen)           # [1, F, 4, L, L], scaled by 0.18215
        mask = latte_amd.known_mask(known.shape, **mask_kw)
        kw = dict(use_fp16=bool(args.get("use_fp16")))
        if conditional:
            y = torch.tensor([label], device=device)
            kw["y"] = torch.cat([y, torch.full_like(y, int(args.num_classes))]) if guided else y
        if guided:
            kw["cfg_scale"] = cli.cfg_scale
        z = torch.randn(known.shape, device=device)
        if guided:
            z = torch.cat([z, z], 0)                                                     # known / mask are doubled by the loop
        out = diffusion.known_sample_loop(fn, z.shape, known, mask, method=cli.method, noise=z, clip_denoised=False, model_kwargs=kw,
                                          resample=cli.resample, device=device)[:1]
        m5 = mask[:, :, None].expand_as(out).to(device)
        known_diff = float((out[m5 == 1] - known[m5 == 1]).abs().max()) if bool((m5 == 1).any()) else 0.0
        result = vae.decode_video_uint8(out)[0].cpu()                                    # [F, S, S, 3]
        shown = (mask[0].repeat_interleave(8, 1).repeat_interleave(8, 2) * 255).to(torch.uint8)[..., None].repeat(1, 1, 1, 3)
        video = torch.cat([frames, shown, result], dim=2).contiguous()                   # input | mask | result
        path = os.path.join(cli.out, f"{name}_{cli.task.replace(':', '_').replace(',', '-')}.mp4")
        latte_amd.write_mp4(path, video, fps=8)
        rec = {"clip": name, "label": label, "task": cli.task, "method": cli.method, "resample": cli.resample,
               "steps": diffusion.num_timesteps, "cfg_scale": cli.cfg_scale, "known_fraction": float(mask.mean()),
               "known_max_abs_diff": known_diff, "video": path}
        print(json.dumps(rec), flush=True)
        results.append(rec)
    return results


def parse(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument("--config", type=str, default=os.path.join(ROOT, "configs", "tiny_sample.yaml"))
    parser.add_argument("--ckpt", type=str, default="")
    parser.add_argument("--random", action="store_true", help="run without weights: re-draw the zero-initialised layers")
    parser.add_argument("--data", type=str, required=True, help='directory of uint8 frame clips .npy [F, H, W, 3], or "synthetic"')
    parser.add_argument("--task", type=str, required=True, help="prefix:K | keyframes:i,j,... | box:y0,x0,y1,x1 (latent pixels)")
    parser.add_argument("--method", type=str, default="ddim", choices=["ddim", "ddpm"])
    parser.add_argument("--resample", type=int, default=1, help="repetitions of every step (RePaint's resampling)")
    parser.add_argument("--steps", type=int, default=50)
    parser.add_argument("--label", type=int, default=None, help="class label (default: the file-name prefix)")
    parser.add_argument("--cfg-scale", type=float, default=1.0)
    parser.add_argument("--out", type=str, default="./sample_videos")
    parser.add_argument("--max-clips", type=int, default=0)
    parser.add_argument("--vae", type=str, default="")
    parser.add_argument("--seed", type=int, default=0)
    cli = parser.parse_args(argv)
    if bool(cli.ckpt) == bool(cli.random):
        parser.error("give exactly one of --ckpt FILE and --random")
    if cli.steps < 2:
        parser.error("--steps must be at least 2")
    if cli.resample < 1:
        parser.error("--resample must be at least 1")
    if cli.data != "synthetic" and not os.path.isdir(cli.data):
        parser.error(f'--data must be a directory of frame clips or "synthetic", got {cli.data!r}')
    conf = latte_amd.load_config(cli.config)
    if cli.label is not None and not 0 <= cli.label < int(conf.num_classes):
        parser.error(f"--label must be in [0, {int(conf.num_classes)})")
    return conf, cli


if __name__ == "__main__":
    main(*parse())
