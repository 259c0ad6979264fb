"""tools/invert.py: the argument checks on the CPU (its parser, in this process), and one end-to-end run on configs/tiny_sample.yaml with random weights and
synthetic clips on the GPU (a fresh child process under a time limit).  The reconstruction MSE is only required to be finite: the
round trip of an untrained model does not come back."""
import json
import math
import os
import subprocess
import sys

import pytest

from _util import ROOT

TOOL = os.path.join(ROOT, "tools", "invert.py")
CONFIG = os.path.join(ROOT, "configs", "tiny_sample.yaml")


def _run(*args, timeout=240):
    return subprocess.run([sys.executable, TOOL, "--config", CONFIG, *args], capture_output=True, text=True, timeout=timeout, cwd=ROOT)


@pytest.mark.parametrize("args,word", [
    (("--data", "synthetic"), "exactly one of --ckpt FILE and --random"),
    (("--data", "synthetic", "--random", "--ckpt", "x.pt"), "exactly one of --ckpt FILE and --random"),
    (("--random",), "--data"),
    (("--random", "--data", "synthetic", "--steps", "1"), "--steps must be at least 2"),
    (("--random", "--data", "/nonexistent/clips"), "--data must be a directory"),
    (("--random", "--data", "synthetic", "--target-label", "101"), "--target-label must be in [0, 101)"),
    (("--random", "--data", "synthetic", "--label", "-1"), "--label must be in [0, 101)"),
])
def test_argument_errors(args, word, capsys):
    import importlib.util
    spec = importlib.util.spec_from_file_location("_invert_tool", TOOL)
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    with pytest.raises(SystemExit) as e:
        tool.parse(["--config", CONFIG, *args])
    assert e.value.code == 2 and word in capsys.readouterr().err


@pytest.mark.gpu
def test_driver_random_weights_synthetic_clips(tmp_path):
    r = _run("--random", "--data", "synthetic", "--steps", "6", "--max-clips", "2", "--label", "3", "--out", str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    recs = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert [x["clip"] for x in recs] == ["synthetic_0", "synthetic_1"]
    for x in recs:
        assert x["label"] == x["target_label"] == 3 and x["steps"] == 6
        assert math.isfinite(x["reconstruction_mse"]) and math.isfinite(x["inverted_std"]) and x["inverted_std"] > 0
        assert os.path.getsize(x["video"]) > 0 and os.path.dirname(x["video"]) == str(tmp_path)
    # another target label under guidance: no reconstruction figure, the doubled batch in both directions
    r = _run("--random", "--data", "synthetic", "--steps", "6", "--max-clips", "1", "--label", "3", "--target-label", "7", "--cfg-scale", "4.0",
             "--out", str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    (x,) = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert x["target_label"] == 7 and "reconstruction_mse" not in x and os.path.getsize(x["video"]) > 0
