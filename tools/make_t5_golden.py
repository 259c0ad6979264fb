"""Writes tests/golden/t5_tiny.npz: ids, masks and the last_hidden_state that ``transformers.T5EncoderModel`` itself computes (fp32, CPU)
for the seeded weights of ``latte_amd.random_init.t5_state_dict``.  Weights are not stored: the file keeps their seed and an abs-sum
checksum, so a test first proves it rebuilt the same weights and then compares against transformers' output without transformers
being installed.

  python tools/make_t5_golden.py
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from latte_amd.random_init import t5_state_dict  # noqa: E402

CFG = dict(d_model=128, d_kv=64, num_heads=4, d_ff=256, num_layers=3, vocab_size=300, relative_attention_num_buckets=32,
           relative_attention_max_distance=128)
SEED = 5


def weight_checksum(sd):
    return float(sum(v.double().abs().sum() for k, v in sorted(sd.items()) if k != "encoder.embed_tokens.weight"))


def main():
    from transformers import T5Config, T5EncoderModel
    torch.manual_seed(0)
    sd = t5_state_dict(SEED, **CFG)
    model = T5EncoderModel(T5Config(feed_forward_proj="gated-gelu", layer_norm_epsilon=1e-6, dropout_rate=0.0, **CFG)).eval()
    model.load_state_dict(sd)
    g = torch.Generator().manual_seed(1)
    B, L = 3, 120
    ids = torch.randint(2, CFG["vocab_size"], (B, L), generator=g)
    mask = torch.ones(B, L, dtype=torch.int64)
    mask[1, 37:] = 0
    mask[2, 1:] = 0
    ids[2, 0] = 1                        # the negative prompt "": EOS alone
    ids[mask == 0] = 0
    with torch.no_grad():
        out = model(input_ids=ids, attention_mask=mask).last_hidden_state
    path = os.path.join(ROOT, "tests", "golden", "t5_tiny.npz")
    np.savez_compressed(path, cfg_json=np.frombuffer(json.dumps(CFG).encode(), dtype=np.uint8), seed=np.int64(SEED),
                        ids=ids.numpy(), mask=mask.numpy(), out=out.numpy().astype(np.float32),
                        weight_abs_sum=np.float64(weight_checksum(sd)))
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
