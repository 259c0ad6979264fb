"""Measures training from stored VAE moments (latte_amd.MomentStore, latte_amd/csrc/moments.hip); writes
profiles/moment_store.json (or --out).  Speed only: no number here says anything about model quality.

  1. Three feeds of LatteTrainer.train_step -- Latte-B/2, local batch 5, f16 operands, 16 x 32 x 32 latents, random weights, one
     process --, interleaved in repetitions of equal step counts (host clock around a window that ends in a device synchronise):
       a  latents already on the device (existing code: the yardstick);
       b  MomentStore.sample_clips from a device-resident f16 store, windows and flips drawn on the host every step;
       c  the existing raw path: per item window + gather on the host, upload, transform launch, AutoencoderKL.encode_video_raw.
     Medians, the per-repetition ratios b / a and c / a, and a's own range over the repetitions.
  2. latte_moment_sample alone at 80 and 120 frames (a micro-batch of 5 x 16 video frames, and with 5 x 8 images): device-event time
     per launch through the C ABI, bytes moved (from the shapes) and achieved bytes/s; with the caller's noise and with the in-kernel draw.
  3. The host-resident store (device="cpu"): gather into pinned memory + upload + launch per batch of 80 frames, synchronised.
  4. store.nbytes of the encoded test clips, and the formula for a real data set.

The store of 1 - 3 is synthetic (random moments, --clips x --frames frames x 2 planes; 512 MiB by default, so the gathered rows come from
HBM, not from a cache a five-clip store would sit in); the store of 4 is built with the encoder from the raw clips of feed c.

  python tools/moment_store_bench.py [--steps 20] [--reps 6]
  rocprofv3 --kernel-trace --stats -d <dir> -- python tools/moment_store_bench.py --trace-feed b     (where feed b's time is)
"""
import argparse
import json
import os
import random
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import latte_amd  # noqa: E402
from latte_amd import video_transforms as vt  # noqa: E402
from latte_amd.random_init import vae_encoder_state_dict  # noqa: E402

B, FR, LAT, HS, WS, S = 5, 16, 32, 240, 320, 256
HW = LAT * LAT


def synthetic_store(clips, frames, dtype=torch.float16):
    g = torch.Generator().manual_seed(0)
    data = [torch.randn(frames, 2, 8, LAT, LAT, generator=g).to(dtype) for _ in range(clips)]
    return latte_amd.MomentStore(data, [f"{i % 101}_clip{i}" for i in range(clips)])


def median(v):
    return float(np.median(v))


def bench_feeds(store, steps, reps, trace_feed=None):
    dev = torch.device("cuda")
    model = latte_amd.Latte_models["Latte-B/2"](input_size=LAT, num_frames=FR, extras=1, max_batch=B).to(dev)
    with torch.no_grad():
        for p in model.parameters():
            if p.requires_grad and float(p.abs().max()) == 0.0:
                p.normal_(0, 0.02)
    tr = latte_amd.LatteTrainer(model, latte_amd.create_diffusion(""), max_batch=B)
    vae = latte_amd.AutoencoderKL(max_frames=FR, with_encoder=True)
    vae.load_state_dict(vae_encoder_state_dict(0))
    vae.to(dev)
    rng = np.random.default_rng(0)
    raw = [rng.integers(0, 256, (40, HS, WS, 3), dtype=np.uint8) for _ in range(B)]
    r = random.Random(0)
    transform = vt.VideoTransform(vt.UCFCenterCropVideo(S), vt.RandomHorizontalFlipVideo(rng=r))
    window = vt.TemporalRandomCrop(FR, rng=r)
    gen = torch.Generator(dev).manual_seed(0)
    fixed = torch.randn(B, FR, 4, LAT, LAT, generator=torch.Generator().manual_seed(1)).to(dev) * 0.18215
    n_clips, frames = store.num_clips, store.clip_frames

    def step_a():
        return tr.train_step(fixed)

    def step_b():                                              # per item: clip, window, flip on the host; one launch for the batch
        clips = [r.randrange(n_clips) for _ in range(B)]
        starts = [window(frames[c])[0] for c in clips]
        flips = transform.draw_flips(B)
        return tr.train_step(store.sample_clips(clips, starts, flips, FR, 1, generator=gen))

    def step_c():                                              # tools/train.py's raw mode
        lat = []
        for a in raw:
            b0, e0 = window(a.shape[0])
            fr = torch.from_numpy(np.ascontiguousarray(a[vt.frame_indices(b0, e0, FR)]))
            lat.append(vae.encode_video_raw(fr.to(dev).unsqueeze(0), transform, generator=gen))
        return tr.train_step(torch.cat(lat))

    feeds = (("a", step_a), ("b", step_b), ("c", step_c))
    for _, fn in feeds:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    if trace_feed:                                             # one window of one feed, for a kernel trace of this process
        for _ in range(steps):
            dict(feeds)[trace_feed]()
        torch.cuda.synchronize()
        return None, None
    ms = {k: [] for k, _ in feeds}
    for _ in range(reps):
        for name, fn in feeds:
            t0 = time.perf_counter()
            for _ in range(steps):
                out = fn()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) / steps * 1e3)
    # host time of feed b's data side alone (draws + row arithmetic + the launch's enqueue), no synchronise inside the window
    t0 = time.perf_counter()
    for _ in range(200):
        clips = [r.randrange(n_clips) for _ in range(B)]
        store.sample_clips(clips, [window(frames[c])[0] for c in clips], transform.draw_flips(B), FR, 1, generator=gen)
    host_b = (time.perf_counter() - t0) / 200 * 1e3
    torch.cuda.synchronize()
    med = {k: median(v) for k, v in ms.items()}
    test_store = latte_amd.MomentStore.build(vae, [(f"{i}_raw{i}", a) for i, a in enumerate(raw)], transform, dtype="f16")
    return {
        "config": "Latte-B/2, local batch 5, f16 operands, 16 x 32 x 32 latents, random weights, one process",
        "steps_per_repetition": steps, "repetitions": reps,
        "ms_per_step": {k: [round(x, 3) for x in v] for k, v in ms.items()},
        "median_ms_per_step": {k: round(v, 3) for k, v in med.items()},
        "median_samples_per_s": {k: round(B / v * 1e3, 1) for k, v in med.items()},
        "ratio_b_over_a_per_repetition": [round(b / a, 4) for a, b in zip(ms["a"], ms["b"])],
        "ratio_c_over_a_per_repetition": [round(c / a, 4) for a, c in zip(ms["a"], ms["c"])],
        "ratio_b_over_a_medians": round(med["b"] / med["a"], 4),
        "ratio_c_over_a_medians": round(med["c"] / med["a"], 4),
        "a_range_over_its_median": [round(min(ms["a"]) / med["a"], 4), round(max(ms["a"]) / med["a"], 4)],
        "b_host_ms_per_batch_enqueue_only": round(host_b, 3),
        "last_loss": float(out["loss"].mean()),
    }, test_store


def bench_kernel(store, launches):
    from latte_amd._lib import check, load_library, ptr, stream_ptr
    import ctypes
    lib, st = load_library(), stream_ptr()
    res = {}
    rng = np.random.default_rng(1)
    for n in (80, 120):
        rows = np.ascontiguousarray(rng.integers(0, store.num_rows, n), dtype=np.int64)
        noise = torch.randn(n, 4, HW, device="cuda")
        out = torch.empty(n, 4, HW, device="cuda")
        rp = ctypes.c_void_p(rows.ctypes.data)
        for label, nz in (("caller_noise", noise), ("in_kernel_draw", None)):
            args = (ptr(store._data), 1, store.num_rows, HW, rp, n, ptr(nz), 7, 0, 0.18215, 2, ptr(out), st)
            for _ in range(20):
                check(lib.latte_moment_sample(*args))
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(launches):
                check(lib.latte_moment_sample(*args))
            e1.record()
            torch.cuda.synchronize()
            us = e0.elapsed_time(e1) * 1e3 / launches
            moved = n * 8 * HW * 2 + n * 4 * HW * 4 * (2 if nz is not None else 1)      # f16 moments + [noise] + out
            res[f"{n}_frames_{label}"] = {"us_per_launch_back_to_back": round(us, 2), "bytes_moved": moved,
                                          "achieved_GB_per_s": round(moved / us / 1e3, 1)}
    return res


def bench_host_store(store, batches):
    host = latte_amd.MomentStore([store._data.cpu().view(-1, 2, 8, LAT, LAT)], ["0_all"], device="cpu")
    rng = np.random.default_rng(2)
    gen = torch.Generator("cuda").manual_seed(0)
    for _ in range(3):
        host.sample_frames(rng.integers(0, host.num_rows, 80), generator=gen)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(batches):
        host.sample_frames(rng.integers(0, host.num_rows, 80), generator=gen)
        torch.cuda.synchronize()
    return {"frames_per_batch": 80, "ms_per_batch_synchronised": round((time.perf_counter() - t0) / batches * 1e3, 3),
            "bytes_uploaded_per_batch": 80 * 8 * HW * 2}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--clips", type=int, default=256)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--launches", type=int, default=2000)
    ap.add_argument("--trace-feed", choices=("a", "b", "c"), default=None,
                    help="warm up, run --steps steps of this feed alone and write nothing: the program of a rocprofv3 --kernel-trace --stats run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "moment_store.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "tools/moment_store_bench.py needs the MI355X"
    assert a.reps >= 5, "at least five repetitions per feed"
    store = synthetic_store(a.clips, a.frames).to("cuda")
    result = {"device": torch.cuda.get_device_name(0),
              "note": "speed only: no number here says anything about model quality",
              "synthetic_store": {"clips": a.clips, "frames_per_clip": a.frames, "planes": 2, "dtype": store.dtype, "nbytes": store.nbytes}}
    if a.trace_feed:
        bench_feeds(store, a.steps, a.reps, a.trace_feed)
        return
    feeds, test_store = bench_feeds(store, a.steps, a.reps)
    result["feeds"] = feeds
    result["kernel"] = bench_kernel(store, a.launches)
    result["host_resident_store"] = bench_host_store(store, 50)
    result["test_store"] = {"clips": test_store.num_clips, "frames": sum(test_store.clip_frames), "planes": len(test_store.planes),
                            "dtype": test_store.dtype, "nbytes": test_store.nbytes}
    result["nbytes_formula"] = "frames x planes x 8 x h x w x (2 for f16 | 4 for fp32) bytes: 32 x 32 latents, f16, both planes = 32 KiB per frame"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
