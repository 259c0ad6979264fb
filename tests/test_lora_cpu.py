"""LoRA fine-tuning, the host side (no GPU): the adapter table of latte_trainer_lora_enable for the training-step fixture's model and
for Latte-XL/2, what the engine and the Python shim refuse, and a torch restatement of the identities the GPU tests
(tests/test_lora_training.py) rest on: with W_eff = W + s B A, dB = s dW A^T and dA = s B^T dW are what autograd gives for A and B,
and they equal the engine's row-wise form dB = dY^T (s x A^T), dA = (s dY B)^T x."""
import ctypes
import math

import pytest
import torch

from latte_amd._lib import ModelConfig, c_i64
from oracle.make_golden import TRAIN_STEP

LINEARS = ("attn.qkv", "attn.proj", "mlp.fc1", "mlp.fc2")


def expected_table(D, Hm, depth, rank, mask):
    shapes = {"attn.qkv": (3 * D, D), "attn.proj": (D, D), "mlp.fc1": (Hm, D), "mlp.fc2": (D, Hm)}
    out, off = [], 0
    for i in range(depth):
        for j, name in enumerate(LINEARS):
            if not mask >> j & 1:
                continue
            n, k = shapes[name]
            for key, numel in ((f"blocks.{i}.{name}.lora_A", rank * k), (f"blocks.{i}.{name}.lora_B", n * rank)):
                out.append((key, off, numel))
                off += (numel + 3) // 4 * 4
    return out, off


def engine_table(lib, cfg, rank, alpha, mask):
    n, total = ctypes.c_int(), c_i64()
    assert lib.latte_debug_lora_table(cfg, rank, alpha, mask, -1, None, 0, None, None, n, total) == 0, lib.latte_last_error()
    rows = []
    buf = ctypes.create_string_buffer(96)
    for i in range(n.value):
        off, numel = c_i64(), c_i64()
        assert lib.latte_debug_lora_table(cfg, rank, alpha, mask, i, buf, 96, off, numel, None, None) == 0, lib.latte_last_error()
        rows.append((buf.value.decode(), off.value, numel.value))
    return rows, total.value


def config(hidden, depth, heads, mlp_ratio=4):
    cfg = ModelConfig()
    cfg.hidden_size, cfg.depth, cfg.num_heads, cfg.mlp_hidden = hidden, depth, heads, mlp_ratio * hidden
    return cfg


@pytest.mark.parametrize("rank,mask", [(8, 15), (4, 1), (32, 10), (16, 6)])
def test_adapter_table_of_the_training_step_fixture(lib, rank, mask):
    cfg = config(TRAIN_STEP["hidden_size"], TRAIN_STEP["depth"], TRAIN_STEP["num_heads"])
    rows, total = engine_table(lib, cfg, rank, float(rank), mask)
    want, want_total = expected_table(128, 512, 2, rank, mask)
    assert rows == want and total == want_total
    assert all(off % 4 == 0 for _, off, _ in rows)                       # 16-byte aligned tensors


def test_adapter_table_of_latte_xl_2(lib):
    cfg = config(1152, 28, 16)
    rows, total = engine_table(lib, cfg, 16, 32.0, 15)
    want, want_total = expected_table(1152, 4608, 28, 16, 15)
    assert rows == want and total == want_total
    assert len(rows) == 28 * 8 and rows[0][0] == "blocks.0.attn.qkv.lora_A" and rows[-1][0] == "blocks.27.mlp.fc2.lora_B"
    # r (K + N) per linear: 16 * (1152 + 3456 + 1152 + 1152 + 1152 + 4608 + 4608 + 1152) floats per block
    assert total == 28 * 16 * 18432 and total * 4 < 34 * 2 ** 20          # the adapters: 31.5 MiB of fp32 against 2.5 GiB of base


def test_the_engine_refuses_bad_ranks_masks_and_alphas(lib):
    cfg = config(128, 2, 2)
    for rank in (0, 1, 3, 12, 48, 64, 128, -4):
        assert lib.latte_debug_lora_table(cfg, rank, 8.0, 15, -1, None, 0, None, None, None, None) != 0
        assert b"rank must be one of 4, 8, 16, 32" in lib.latte_last_error()
    assert lib.latte_debug_lora_table(cfg, 64, 8.0, 15, -1, None, 0, None, None, None, None) != 0
    assert b"rank 64 is not offered" in lib.latte_last_error()        # the kernels take it; its step measured slower than the full step
    for mask in (0, 16, -1, 31):
        assert lib.latte_debug_lora_table(cfg, 8, 8.0, mask, -1, None, 0, None, None, None, None) != 0
        assert b"non-empty subset" in lib.latte_last_error()
    for alpha in (0.0, -1.0, float("inf"), float("nan")):
        assert lib.latte_debug_lora_table(cfg, 8, alpha, 15, -1, None, 0, None, None, None, None) != 0
        assert b"alpha must be positive" in lib.latte_last_error()
    # entry points that need a bound LoRA trainer answer a null handle with an error, not a crash
    assert lib.latte_trainer_lora_enable(None, 8, 8.0, 15) != 0
    assert lib.latte_trainer_bind_lora(None, None, None, None, None, None, None) != 0
    assert lib.latte_trainer_lora_merge(None, None, None, None) != 0
    assert lib.latte_trainer_lora_num_params(None) == 0 and lib.latte_trainer_lora_total_numel(None) == 0
    assert lib.latte_trainer_lora_param_key(None, 0) is None and lib.latte_trainer_lora_param_offset(None, 0) == -1


def test_target_names_map_to_the_mask():
    from latte_amd import LatteError
    from latte_amd.training import LORA_TARGETS, lora_target_mask
    assert LORA_TARGETS == ("qkv", "proj", "fc1", "fc2")
    assert lora_target_mask(LORA_TARGETS) == 15 and lora_target_mask(("fc2", "qkv")) == 9 and lora_target_mask("proj, fc1") == 6
    for bad in ((), ("q",), "qkv,out", ""):
        with pytest.raises(LatteError):
            lora_target_mask(bad)


def test_projection_identities():
    """y = x (W + s B A)^T: autograd's dA and dB are the projections s B^T dW and s dW A^T of the merged weight's gradient dW = dY^T x
    -- the GPU tests' reference -- and the row-wise products the engine forms."""
    g = torch.Generator().manual_seed(3)
    M, N, K, r, s = 48, 24, 40, 8, 2.0
    x = torch.randn(M, K, generator=g, dtype=torch.float64)
    W = torch.randn(N, K, generator=g, dtype=torch.float64)
    A = torch.randn(r, K, generator=g, dtype=torch.float64).requires_grad_()
    B = torch.randn(N, r, generator=g, dtype=torch.float64).requires_grad_()
    dY = torch.randn(M, N, generator=g, dtype=torch.float64)
    y = x @ (W + s * B @ A).T
    dA, dB = torch.autograd.grad(y, [A, B], dY)
    dW = dY.T @ x
    assert torch.allclose(dB, s * dW @ A.T.detach(), rtol=1e-12, atol=1e-12)
    assert torch.allclose(dA, s * B.T.detach() @ dW, rtol=1e-12, atol=1e-12)
    h, gg = s * x @ A.T.detach(), s * dY @ B.detach()
    assert torch.allclose(dB, dY.T @ h, rtol=1e-12, atol=1e-12)
    assert torch.allclose(dA, gg.T @ x, rtol=1e-12, atol=1e-12)
    # the initial state B = 0: dA vanishes identically, which is why the gradient tests draw a non-zero B
    assert float((s * torch.zeros(N, r, dtype=torch.float64).T @ dW).abs().max()) == 0.0
    # kaiming-uniform with a = sqrt(5) is U(-1 / sqrt(K), 1 / sqrt(K)): nn.Linear's own init
    a = torch.empty(r, 4096)
    torch.nn.init.kaiming_uniform_(a, a=math.sqrt(5))
    assert float(a.abs().max()) <= 1 / 64 and float(a.abs().max()) > 0.99 / 64
