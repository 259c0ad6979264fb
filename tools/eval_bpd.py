"""Held-out likelihood of a checkpoint in bits per dimension: GaussianDiffusion.calc_bpd_loop (gaussian_diffusion.py:813-866) on the
MI355X engine -- the one evaluation metric of the reference that needs no detector network.

  python tools/eval_bpd.py --config configs/tiny_sample.yaml [--ckpt model.pt] --data DIR|synthetic [--batch 8]
                           [--clip-denoised | --no-clip-denoised] [--seed 0] [--respacing ""] [--max-clips N]

The model comes from a sample YAML exactly as tools/sample.py builds it (config -> get_models -> find_model, "ema" preferred);
without --ckpt the zero-initialised adaLN / final layers are re-drawn so the run exercises the whole path (plumbing, not a number
worth quoting).  --data is a directory of latent clips (.npy [F, 4, h, w], already scaled by 0.18215, as tools/encode_clips.py
writes them; label = file-name prefix, as tools/train.py reads it) or "synthetic" (N(0, 1) latents clamped to [-1, 1]).  The whole
chain of a batch is ONE latte_bpd_loop call (latte_amd.SpacedDiffusion.calc_bpd_loop with model.forward); its noise comes from the
engine's Philox stream, seeded with --seed.  --respacing "" is the full chain (1000 steps), the variational bound itself; a
respacing such as "50" gives a quick, coarser figure.

Prints one JSON line per batch and a final one: mean and standard error over clips of total_bpd and prior_bpd, and the vb /
xstart_mse / mse tables averaged over clips (column 0 = t = T-1)."""
import argparse
import glob
import json
import math
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


def batches(cli, args):
    """-> iterator of (x0 [n, F, 4, h, w] float32, labels int64[n])"""
    shape = (args.num_frames, 4, args.latent_size, args.latent_size)
    if cli.data == "synthetic":
        g = torch.Generator("cpu").manual_seed(cli.seed)
        total = cli.max_clips or 2 * cli.batch
        for lo in range(0, total, cli.batch):
            n = min(cli.batch, total - lo)
            yield torch.randn(n, *shape, generator=g).clamp(-1.0, 1.0), torch.randint(0, max(int(args.num_classes), 1), (n,), generator=g)
        return
    files = sorted(glob.glob(os.path.join(cli.data, "*.npy")))
    if not files:
        raise SystemExit(f"no .npy latent clips under {cli.data}")
    if cli.max_clips:
        files = files[:cli.max_clips]
    for lo in range(0, len(files), cli.batch):
        xs = []
        for f in files[lo:lo + cli.batch]:
            a = np.load(f)
            if a.dtype == np.uint8 or tuple(a.shape[1:]) != shape[1:] or a.shape[0] < shape[0]:
                raise SystemExit(f"{f}: expected a latent clip [F >= {shape[0]}, 4, {shape[2]}, {shape[3]}] (tools/encode_clips.py), "
                                 f"got {a.dtype} {tuple(a.shape)}")
            xs.append(torch.from_numpy(np.ascontiguousarray(a[:shape[0]], dtype=np.float32)))
        yield torch.stack(xs), torch.tensor([clip_label(f) for f in files[lo:lo + cli.batch]], dtype=torch.int64)


def mean_sem(v):
    v = np.asarray(v, dtype=np.float64)
    return float(v.mean()), float(v.std(ddof=1) / math.sqrt(len(v))) if len(v) > 1 else 0.0


def main(args, cli):
    torch.manual_seed(cli.seed)
    torch.set_grad_enabled(False)
    if not torch.cuda.is_available():
        raise SystemExit("tools/eval_bpd.py needs an MI355X (latte_amd has no CPU fallback)")
    args.latent_size = args.image_size // 8
    args.max_batch = cli.batch
    model = get_models(args).to("cuda")
    if args.get("ckpt"):
        model.load_state_dict(find_model(args.ckpt))
    else:
        g = torch.Generator("cpu").manual_seed(1)
        for _, p in model.named_parameters():
            if p.requires_grad and float(p.detach().abs().max()) == 0.0:
                p.copy_(torch.randn(p.shape, generator=g) * 0.02)
        model.mark_weights_dirty()
    model.eval()
    if args.get("use_fp16"):
        model.to(dtype=torch.float16)
    diffusion = create_diffusion(cli.respacing, learn_sigma=bool(args.learn_sigma))
    model.set_engine_option("seed", cli.seed, batch=cli.batch)
    per_clip = {"total_bpd": [], "prior_bpd": []}
    sums, labels_seen, clips = {}, [], 0
    for bi, (x0, y) in enumerate(batches(cli, args)):
        kwargs = dict(y=y.cuda()) if int(args.extras) == 2 else {}
        r = diffusion.calc_bpd_loop(model.forward, x0.cuda(), clip_denoised=cli.clip_denoised, model_kwargs=kwargs)
        r = {k: v.double().cpu().numpy() for k, v in r.items()}
        for k in per_clip:
            per_clip[k] += r[k].tolist()
        for k in ("vb", "xstart_mse", "mse"):
            sums[k] = sums.get(k, 0.0) + r[k].sum(axis=0)
        clips += len(y)
        labels_seen += y.tolist()
        print(json.dumps({"batch": bi, "clips": len(y), "labels": y.tolist(), "total_bpd": r["total_bpd"].tolist(),
                          "prior_bpd": r["prior_bpd"].tolist()}), flush=True)
    total, prior = mean_sem(per_clip["total_bpd"]), mean_sem(per_clip["prior_bpd"])
    final = {"clips": clips, "num_timesteps": diffusion.num_timesteps, "clip_denoised": bool(cli.clip_denoised), "seed": cli.seed,
             "labels": labels_seen, "total_bpd": total[0], "total_bpd_sem": total[1], "prior_bpd": prior[0], "prior_bpd_sem": prior[1],
             "vb": (sums["vb"] / clips).tolist(), "xstart_mse": (sums["xstart_mse"] / clips).tolist(), "mse": (sums["mse"] / clips).tolist()}
    print(json.dumps(final), flush=True)
    return final


if __name__ == "__main__":
    parser = argparse.ArgumentParser()
    parser.add_argument("--config", type=str, default=os.path.join(ROOT, "configs", "tiny_sample.yaml"))
    parser.add_argument("--ckpt", type=str, default="")
    parser.add_argument("--data", type=str, required=True, help='directory of latent clips .npy [F, 4, h, w], or "synthetic"')
    parser.add_argument("--batch", type=int, default=2)
    parser.add_argument("--clip-denoised", dest="clip_denoised", action="store_true", default=True)
    parser.add_argument("--no-clip-denoised", dest="clip_denoised", action="store_false")
    parser.add_argument("--seed", type=int, default=0)
    parser.add_argument("--respacing", type=str, default="", help='timestep_respacing of create_diffusion; "" = the full chain')
    parser.add_argument("--max-clips", type=int, default=0)
    cli = parser.parse_args()
    conf = latte_amd.load_config(cli.config)
    if cli.ckpt:
        conf.ckpt = cli.ckpt
    main(conf, cli)
