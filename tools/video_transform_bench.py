"""Measures the video preprocessing launch (latte_amd/csrc/video.hip) and what it costs the training step; writes
profiles/video_transform.json (or --out).

  1. latte_video_transform for 16 x 240 x 320 -> 256 (UCFCenterCropVideo): device-event time per launch over a window of launches,
     achieved bytes/s (source bytes inside the window the crop keeps + fp32 output bytes, from the shapes), the worst max-abs
     difference to torch on the CPU over the test shapes;
  2. the same Compose (ToTensorVideo, UCFCenterCropVideo, Normalize) on the host with torch at 16 threads;
  3. training samples/s of BASELINE config 5 (Latte-B/2, 16 x 256 x 256, local batch 5, random weights) with the VAE encode in the
     loop: raw clips (window + gather on the host, upload, transform, encode) beside pre-cut 256 x 256 frame clips (upload, encode),
     alternated in the same process.

  python tools/video_transform_bench.py [--steps 15] [--rounds 2] [--skip-train]
"""
import argparse
import json
import os
import random
import sys
import tempfile
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import latte_amd  # noqa: E402
from latte_amd import video_transforms as vt  # noqa: E402
from latte_amd.random_init import vae_encoder_state_dict  # noqa: E402

N, HS, WS, S = 16, 240, 320, 256


def host_compose(frames, size):
    """ToTensorVideo -> UCFCenterCropVideo(size) -> Normalize(0.5, 0.5) in torch on the CPU; frames uint8 [N, Hs, Ws, 3]."""
    x = frames.permute(0, 3, 1, 2).float() / 255.0
    h, w = x.shape[-2:]
    x = F.interpolate(x, scale_factor=size / min(h, w), mode="bilinear", align_corners=False)
    h, w = x.shape[-2:]
    i, j = int(round((h - size) / 2.0)), int(round((w - size) / 2.0))
    return x[..., i:i + size, j:j + size].contiguous().sub_(0.5).div_(0.5)


def host_sky(frames, size):
    """ToTensorVideo -> CenterCropResizeVideo(size) -> Normalize(0.5, 0.5) in torch on the CPU."""
    x = frames.permute(0, 3, 1, 2).float() / 255.0
    h, w = x.shape[-2:]
    i, j = (0, int(round((w - h) / 2.0))) if h < w else (int(round((h - w) / 2.0)), 0)
    x = x[..., i:i + min(h, w), j:j + min(h, w)]
    return F.interpolate(x, size=(size, size), mode="bilinear", align_corners=False).contiguous().sub_(0.5).div_(0.5)


def bench_kernel(launches):
    g = torch.Generator().manual_seed(0)
    x = torch.randint(0, 256, (N, HS, WS, 3), generator=g, dtype=torch.uint8)
    xd = x.cuda()
    t = vt.VideoTransform(vt.UCFCenterCropVideo(S))
    for _ in range(20):
        out = t(xd)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    # the launch alone through the C ABI into one output buffer (the Python wrapper's allocation and checks cost more host time than
    # the kernel runs, and would be what a back-to-back window measures)
    from latte_amd._lib import check, load_library, ptr, stream_ptr
    lib, st = load_library(), stream_ptr()
    src_p, out_p, none_p = ptr(xd), ptr(out), ptr(None)
    e0.record()
    for _ in range(launches):
        check(lib.latte_video_transform(src_p, N, HS, WS, vt.KIND_UCF_CENTER_CROP, S, S, none_p, out_p, st))
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / launches
    t0 = time.perf_counter()
    for _ in range(launches):
        out = t(xd)
    torch.cuda.synchronize()
    wrapper_us = (time.perf_counter() - t0) / launches * 1e6
    p = vt.plan(vt.KIND_UCF_CENTER_CROP, HS, WS, S, S)
    # source bytes the kept window covers (all rows; crop_j .. crop_j + S intermediate columns), and the fp32 output
    cols = min(WS, int(np.ceil((p.crop_j + S) * p.scale_w)) + 1) - int(p.crop_j * p.scale_w)
    read = N * HS * cols * 3
    written = N * 3 * S * S * 4
    err = float((out.cpu() - host_compose(x, S)).abs().max())
    # worst difference over the shapes of tests/test_video_transforms_gpu.py, all three kinds
    worst = err
    for n, hs, ws, s in [(2, 300, 200, 128), (1, 512, 512, 256), (1, 5, 7, 8), (2, 40, 27, 18), (6, 37, 53, 16)]:
        y = torch.randint(0, 256, (n, hs, ws, 3), generator=g, dtype=torch.uint8)
        worst = max(worst, float((vt.VideoTransform(vt.UCFCenterCropVideo(s))(y.cuda()).cpu() - host_compose(y, s)).abs().max()))
    for n, hs, ws, s in [(3, 180, 320, 128), (2, 45, 28, 24), (1, 31, 36, 13), (6, 37, 53, 16)]:
        y = torch.randint(0, 256, (n, hs, ws, 3), generator=g, dtype=torch.uint8)
        worst = max(worst, float((vt.VideoTransform(vt.CenterCropResizeVideo(s))(y.cuda()).cpu() - host_sky(y, s)).abs().max()))
    y = torch.randint(0, 256, (2, 30, 50, 3), generator=g, dtype=torch.uint8)
    taichi = (y.permute(0, 3, 1, 2).float() / 255.0).flip(-1).contiguous().sub_(0.5).div_(0.5)
    worst = max(worst, float((vt.VideoTransform(None)(y.cuda(), flip=True).cpu() - taichi).abs().max()))
    torch.set_num_threads(16)
    for _ in range(3):
        host_compose(x, S)
    t0 = time.perf_counter()
    reps = 20
    for _ in range(reps):
        host_compose(x, S)
    host_ms = (time.perf_counter() - t0) / reps * 1e3
    return {"shape": f"{N} x {HS} x {WS} -> {S} (UCFCenterCropVideo)", "launches_timed": launches, "us_per_launch_back_to_back": round(us, 2), "us_per_call_python_wrapper": round(wrapper_us, 2),
            "bytes_read": read, "bytes_written": written, "achieved_GB_per_s": round((read + written) / us / 1e3, 1),
            "max_abs_vs_torch_cpu_headline": err, "max_abs_vs_torch_cpu_worst": worst,
            "host_torch_16_threads_ms": round(host_ms, 2), "host_frames_per_s": round(N / host_ms * 1e3, 1),
            "gpu_frames_per_s": round(N / us * 1e6, 1)}


def bench_train(steps, rounds):
    B, FR = 5, 16
    dev = torch.device("cuda")
    model = latte_amd.Latte_models["Latte-B/2"](input_size=32, num_frames=FR, extras=1, max_batch=B).to(dev)
    with torch.no_grad():
        for p in model.parameters():
            if p.requires_grad and float(p.abs().max()) == 0.0:
                p.normal_(0, 0.02)
    tr = latte_amd.LatteTrainer(model, latte_amd.create_diffusion(""), max_batch=B)
    vae = latte_amd.AutoencoderKL(max_frames=FR, with_encoder=True)
    vae.load_state_dict(vae_encoder_state_dict(0))
    vae.to(dev)
    rng = np.random.default_rng(0)
    tmp = tempfile.mkdtemp(prefix="vt_bench_")
    raw, cut = [], []
    for i in range(B):
        np.save(os.path.join(tmp, f"raw{i}.npy"), rng.integers(0, 256, (40, HS, WS, 3), dtype=np.uint8))
        np.save(os.path.join(tmp, f"cut{i}.npy"), rng.integers(0, 256, (FR, S, S, 3), dtype=np.uint8))
        raw.append(np.load(os.path.join(tmp, f"raw{i}.npy"), mmap_mode="r"))
        cut.append(os.path.join(tmp, f"cut{i}.npy"))
    r = random.Random(0)
    transform = vt.VideoTransform(vt.UCFCenterCropVideo(S), vt.RandomHorizontalFlipVideo(rng=r))
    window = vt.TemporalRandomCrop(FR, rng=r)
    gen = torch.Generator(dev).manual_seed(0)
    host_s = [0.0]

    def step_raw():
        lat = []
        for a in raw:                                          # as tools/train.py's raw mode: per item window, gather, upload, transform, encode
            t0 = time.perf_counter()
            b, e = window(a.shape[0])
            fr = torch.from_numpy(np.ascontiguousarray(a[vt.frame_indices(b, e, FR)]))
            host_s[0] += time.perf_counter() - t0
            lat.append(vae.encode_video_raw(fr.to(dev).unsqueeze(0), transform, generator=gen))
        return tr.train_step(torch.cat(lat))

    def step_cut():                                            # as tools/train.py's frame-clip mode: load, stack, upload, encode
        t0 = time.perf_counter()
        x = torch.stack([torch.from_numpy(np.load(f)) for f in cut])
        host_s[0] += time.perf_counter() - t0
        return tr.train_step(vae.encode_video_uint8(x.to(dev), generator=gen))

    res = {"raw": [], "frames": []}
    host = {"raw": [], "frames": []}
    for fn in (step_raw, step_cut):
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for name, fn in (("raw", step_raw), ("frames", step_cut)):
            host_s[0] = 0.0
            t0 = time.perf_counter()
            for _ in range(steps):
                out = fn()
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / steps
            res[name].append(round(B / dt, 2))
            host[name].append(round(host_s[0] / steps * 1e3, 2))
    for f in os.listdir(tmp):
        os.unlink(os.path.join(tmp, f))
    os.rmdir(tmp)
    return {"config": "Latte-B/2, 16 x 256 x 256, local batch 5, VAE encode in the loop, random weights", "steps_per_window": steps,
            "samples_per_s_raw_clips_40x240x320": res["raw"], "samples_per_s_frame_clips_16x256x256": res["frames"],
            "host_ms_per_step_read_and_gather_raw": host["raw"], "host_ms_per_step_read_frames": host["frames"],
            "raw_over_frames": round(float(np.mean(res["raw"]) / np.mean(res["frames"])), 4), "last_loss": float(out["loss"].mean())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=3000)
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--skip-train", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "video_transform.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "tools/video_transform_bench.py needs the MI355X"
    result = {"device": torch.cuda.get_device_name(0), "kernel": bench_kernel(a.launches)}
    if not a.skip_train:
        result["training"] = bench_train(a.steps, a.rounds)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
