"""tools/train.py with `lora_rank:` in the config: the frozen base comes from `pretrained:`, a checkpoint of the run is `<step>.lora.pt`
(adapters, their EMA, the LoRA settings) with the state files beside it, and `resume_from_checkpoint: True` continues bit for bit."""
import os
import re
import shutil
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def config(tmp_path, name, **keys):
    text = open(os.path.join(ROOT, "configs", "tiny_train.yaml")).read()
    for k, v in keys.items():
        line = f"{k}: {v}"
        text, n = re.subn(rf"(?m)^{k}:.*$", line, text)
        if not n:
            text += line + "\n"
    path = str(tmp_path / name)
    open(path, "w").write(text)
    return path


def run(cfg, out):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "train.py"), "--config", cfg, "--out", out], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout


def test_train_driver_lora_run_and_exact_resume(tmp_path):
    import latte_amd
    # the checkpoint to fine-tune: the tiny config's model with drawn weights, in the reference's {"model", "ema"} format
    m = latte_amd.Latte_models["Latte-S/2"](input_size=8, num_frames=4, num_classes=5, extras=2, learn_sigma=True)
    g = torch.Generator("cpu").manual_seed(9)
    with torch.no_grad():
        for p in m.parameters():
            if p.requires_grad and float(p.abs().max()) == 0.0:
                p.copy_(torch.randn(p.shape, generator=g) * 0.02)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    base = str(tmp_path / "0000002.pt")
    torch.save({"model": sd, "ema": sd}, base)
    keys = dict(pretrained=f'"{base}"', lora_rank=8, lora_alpha=16, lora_targets='"qkv,fc2"', max_train_steps=6, ckpt_every=3, log_every=2)
    out = str(tmp_path / "run")
    log = run(config(tmp_path, "lora.yaml", **keys), out)
    assert "LoRA: rank 8, alpha 16, targets qkv,fc2" in log and "Train Loss" in log and "0000006.lora.pt" in log
    ck = os.path.join(out, "checkpoints")
    assert sorted(os.listdir(ck)) == ["0000003.lora.pt", "0000003.state.pt", "0000006.lora.pt", "0000006.state.pt"]   # the step count went on from 2
    full = torch.load(os.path.join(ck, "0000006.lora.pt"))
    assert set(full) == {"config", "lora", "lora_ema"} and full["config"] == {"lora_rank": 8, "lora_alpha": 16.0, "lora_targets": ["qkv", "fc2"]}
    assert len(full["lora"]) == 12 * 2 * 2 and full["lora"]["blocks.0.attn.qkv.lora_A"].shape == (8, 384)                # Latte-S: depth 12, D 384
    assert float(full["lora"]["blocks.11.mlp.fc2.lora_B"].abs().max()) > 0.0
    assert any(not torch.equal(full["lora"][k], full["lora_ema"][k]) for k in full["lora"])
    assert os.path.getsize(os.path.join(ck, "0000006.lora.pt")) < 3 * 2 ** 20      # adapters + their EMA: 2 x 8 x 3456 x 12 floats; the base is 130 MB
    # a second run directory holding the step-3 files only, resumed: steps 4 .. 6 again, the same bits
    out2 = str(tmp_path / "resumed")
    os.makedirs(os.path.join(out2, "checkpoints"))
    for f in ("0000003.lora.pt", "0000003.state.pt"):
        shutil.copy(os.path.join(ck, f), os.path.join(out2, "checkpoints", f))
    log2 = run(config(tmp_path, "resume.yaml", resume_from_checkpoint=True, **keys), out2)
    assert "Resumed from" in log2 and "step 3" in log2
    again = torch.load(os.path.join(out2, "checkpoints", "0000006.lora.pt"))
    for part in ("lora", "lora_ema"):
        for k, v in full[part].items():
            assert torch.equal(v, again[part][k]), (part, k)
    # the file merges into the base on a state dict (tools/sample.py --lora) as the trainer merges it, to fp32 rounding
    from latte_amd.training import merge_lora_state_dict
    msd = merge_lora_state_dict(sd, full["lora"], full["config"])
    w = "blocks.3.attn.qkv.weight"
    want = sd[w] + 2.0 * full["lora"]["blocks.3.attn.qkv.lora_B"] @ full["lora"]["blocks.3.attn.qkv.lora_A"]
    assert torch.equal(msd[w], want) and not torch.equal(msd[w], sd[w]) and torch.equal(msd["blocks.3.attn.proj.weight"], sd["blocks.3.attn.proj.weight"])
