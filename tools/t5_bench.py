"""Times the T5 v1.1 text encoder of text-to-video on the MI355X engine: XXL shape, random weights, B = 2 x L = 120 and B = 1.

  python tools/t5_bench.py [--layers 24] [--iters 10] [--out profiles/t5_bench.json] [--torch-fp16]

Reports ms per encode, the effective weight bytes per second (the bytes of the packed weights one encode reads / time) against
the 8 TB/s HBM figure the README uses, and the weight-streaming floor: the same bytes at the bandwidth a device-to-device copy
of 1 GiB reaches on this GPU.  `--once B` runs a single encode after a warm-up (the workload for a kernel trace).
`--torch-fp16` also times transformers' own fp16 encode of the same shape with random weights, as context only."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import latte_amd  # noqa: E402
from latte_amd.random_init import t5_keys, t5_state_dict  # noqa: E402


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts.sort()
    return ts[len(ts) // 2], ts[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--once", type=int, default=0)
    ap.add_argument("--torch-fp16", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "t5_bench needs an MI355X"
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    cfg = dict(num_layers=a.layers)
    ks = t5_keys(**cfg)
    proj_params = sum(s[0] * s[1] for k, s in ks.items() if len(s) == 2 and "block" in k and "relative" not in k)
    weight_bytes = proj_params * 4                      # the f16 pair: 2 x 2 bytes per weight, read once per encode
    t0 = time.time()
    m = latte_amd.T5EncoderModel(max_batch=2, max_len=120, **cfg).load_state_dict(t5_state_dict(0, **cfg))
    g = torch.Generator().manual_seed(0)
    ids = torch.randint(2, 32128, (2, 120), generator=g).cuda()
    mask = torch.ones(2, 120, dtype=torch.int64)
    mask[1, 20:] = 0
    mask = mask.cuda()
    m(ids, attention_mask=mask)
    torch.cuda.synchronize()
    print(f"built, loaded and packed in {time.time() - t0:.1f} s", flush=True)
    if a.once:
        m(ids[:a.once], attention_mask=mask[:a.once])
        torch.cuda.synchronize()
        return
    src = torch.empty(1 << 30, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    copy_ms, _ = timed(lambda: dst.copy_(src), 10)
    copy_bw = 2 * (1 << 30) / (copy_ms * 1e-3)           # read + write
    res = {"layers": a.layers, "weight_bytes_per_encode": weight_bytes, "copy_bandwidth_TBps": copy_bw / 1e12,
           "weight_streaming_floor_ms": weight_bytes / copy_bw * 1e3, "hbm_TBps_reference": 8.0}
    for B in (2, 1):
        med, best = timed(lambda: m(ids[:B], attention_mask=mask[:B]), a.iters)
        res[f"B{B}_L120"] = {"ms_median": med, "ms_min": best, "effective_weight_TBps": weight_bytes / (med * 1e-3) / 1e12,
                             "fraction_of_8TBps": weight_bytes / (med * 1e-3) / 8e12,
                             "times_the_floor": med / res["weight_streaming_floor_ms"]}
    if a.torch_fp16:
        try:
            from transformers import T5Config, T5EncoderModel
            with torch.device("cuda"):
                hf = T5EncoderModel(T5Config(d_model=4096, d_kv=64, num_heads=64, d_ff=10240, num_layers=a.layers, vocab_size=32128,
                                             feed_forward_proj="gated-gelu")).half().eval()
            with torch.no_grad():
                med, best = timed(lambda: hf(input_ids=ids, attention_mask=mask), a.iters)
            res["transformers_fp16_B2_L120_context_only"] = {"ms_median": med, "ms_min": best}
        except Exception as e:          # context only
            res["transformers_fp16_B2_L120_context_only"] = {"error": repr(e)[:200]}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
