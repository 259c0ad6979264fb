"""tools/eval_bpd.py end to end on configs/tiny_sample.yaml with random weights (no checkpoint): synthetic data, and a directory of
latent clips whose labels come from the file-name prefix.  Each run is a fresh child process under a time limit."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from _util import ROOT

pytestmark = pytest.mark.gpu
KEYS = ("total_bpd", "prior_bpd", "vb", "xstart_mse", "mse")


def _run(*extra):
    cmd = [sys.executable, os.path.join(ROOT, "tools", "eval_bpd.py"), "--config", os.path.join(ROOT, "configs", "tiny_sample.yaml"),
           "--respacing", "20", "--batch", "2", "--seed", "4", *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    return lines[:-1], lines[-1]


def _flat(v):
    return [v] if isinstance(v, float) else list(v)


def _check_final(final, clips):
    assert set(KEYS) <= set(final) and final["clips"] == clips and final["num_timesteps"] == 20
    for k in KEYS:
        assert all(math.isfinite(x) for x in _flat(final[k])), k
    assert len(final["vb"]) == len(final["mse"]) == len(final["xstart_mse"]) == 20
    assert final["total_bpd"] > 0 and final["total_bpd_sem"] >= 0


def test_driver_on_synthetic_data():
    per_batch, final = _run("--data", "synthetic", "--max-clips", "3")
    assert [b["clips"] for b in per_batch] == [2, 1]
    _check_final(final, 3)
    assert final["clip_denoised"] is True


def test_driver_reads_clips_and_labels(tmp_path):
    g = np.random.default_rng(0)
    for name in ("7_a.npy", "12_b.npy", "clip.npy"):
        np.save(tmp_path / name, g.standard_normal((4, 4, 16, 16)).clip(-1, 1).astype(np.float32))
    per_batch, final = _run("--data", str(tmp_path), "--no-clip-denoised")
    assert final["labels"] == [12, 7, 0]          # sorted file names: 12_b, 7_a, clip (no numeric prefix -> 0)
    assert sum(b["clips"] for b in per_batch) == 3
    _check_final(final, 3)
    assert final["clip_denoised"] is False
