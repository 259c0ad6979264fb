"""Measures the parity of latte_amd.T5EncoderModel against the fp32 restatement (tests/t5_reference.py) at the cases of
tests/test_t5_gpu.py and writes them, with the CPU emulation of the operand scheme, to a JSON file.

  python tools/t5_parity.py --out profiles/t5_parity.json"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import latte_amd  # noqa: E402
import t5_reference as R  # noqa: E402
from latte_amd.random_init import t5_state_dict  # noqa: E402

CASES = {"w256_d2": dict(d_model=256, num_heads=4, d_ff=640, num_layers=2, vocab_size=1000),
         "w512_d24": dict(d_model=512, num_heads=8, d_ff=1280, num_layers=24, vocab_size=1000),
         "w1024_d24": dict(d_model=1024, num_heads=16, d_ff=2560, num_layers=24, vocab_size=1000),
         "xxl_d2": dict(d_model=4096, num_heads=64, d_ff=10240, num_layers=2, vocab_size=1000)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    res = {"metric": "relative L2 of last_hidden_state against the fp32 restatement, B = 3 x L = 120 (full, 37 valid, 1 valid)",
           "compute_dtype": "f16", "cases": {}}
    for name, cfg in CASES.items():
        sd = t5_state_dict(3, **cfg)
        g = torch.Generator().manual_seed(11)
        ids = torch.randint(2, cfg["vocab_size"], (3, 120), generator=g)
        mask = torch.ones(3, 120, dtype=torch.int64)
        mask[1, 37:] = 0
        mask[2, 1:] = 0
        want = R.t5_encoder_forward(sd, ids, mask)
        m = latte_amd.T5EncoderModel(cfg, max_batch=3).load_state_dict(sd)
        got = m(ids.cuda(), attention_mask=mask.cuda()).last_hidden_state.cpu()
        row = ((got.double() - want.double()).norm(dim=-1) / want.double().norm(dim=-1)).max().item()
        c = {"engine": R.rel_l2(got, want), "engine_worst_row": row}
        if cfg["d_model"] <= 1024:
            c["cpu_emulation_engine_scheme"] = R.rel_l2(R.t5_encoder_forward(sd, ids, mask, emulate=R.T5_EMULATE_ENGINE), want)
            c["cpu_emulation_all_f16"] = R.rel_l2(R.t5_encoder_forward(sd, ids, mask, emulate=R.T5_EMULATE_ALL), want)
        res["cases"][name] = c
        print(name, json.dumps(c), flush=True)
        del m
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
