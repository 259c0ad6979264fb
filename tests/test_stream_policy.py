"""Cache-policy hints on the once-used streams of a block (engine option "stream_policy"): fc1's hidden stores,
the A-operand DMA of fc2 and of the out-projection, and the fused attention kernel's output stores can be issued `nt`.  A hint is a
template argument of its kernel and changes no value: every hinted form is compared bit for bit with its plain twin."""
import pytest
import torch

import latte_amd
from latte_amd._lib import check, ptr, stream_ptr

pytestmark = pytest.mark.gpu
TD = {0: torch.bfloat16, 1: torch.float16}
FC1_STORE, FC2_A, ATTN_STORE, PROJ_A, ALL = 1, 2, 4, 8, 15   # the option's bits
PLAIN = 16                                                   # latte_debug_set_choice("stream_policy", 16 + mask); 0 = the library's default


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda")


@pytest.fixture
def policy(lib):
    def choose(mask):
        check(lib.latte_debug_set_choice(b"stream_policy", PLAIN + int(mask)))
    yield choose
    check(lib.latte_debug_set_choice(b"stream_policy", 0))


def _operands(M, N, K, dt, dev, seed):
    g = torch.Generator("cpu").manual_seed(seed)
    Mp = (M + 255) // 256 * 256 + 256          # one whole tile of padding rows behind the last (partial) tile
    A = torch.randn(Mp, K, generator=g).to(dev).to(TD[dt])
    W = (torch.randn(N, K, generator=g) / K ** 0.5).to(dev).to(TD[dt])
    bias = torch.randn(N, generator=g).to(dev)
    return Mp, A, W, bias


@pytest.mark.parametrize("dt", [0, 1], ids=["bf16", "f16"])
@pytest.mark.parametrize("M", [256, 300], ids=["single_tile", "clamped_last_tile"])
def test_fc1_hinted_stores_equal_plain(lib, dev, policy, M, dt):
    """gemm_pps_kernel<256, EPI_BIAS_GELU_H16> (variant 9, epi 1): the `nt` stores behind the LDS patch write the same halves to the
    same rows, and no row beyond M (the padding rows keep their sentinel)."""
    N, K = 256, 128
    Mp, A, W, bias = _operands(M, N, K, dt, dev, seed=M + N + K)
    want = torch.nn.functional.gelu(A[:M].float() @ W.float().t() + bias, approximate="tanh")
    outs = {}
    for mask in (0, FC1_STORE):
        policy(mask)
        out = torch.full((Mp, N), -7.0, dtype=TD[dt], device=dev)
        check(lib.latte_debug_gemm(ptr(A), ptr(W), ptr(bias), ptr(out), None, M, N, K, 0, M, 1, dt, 9, stream_ptr()))
        torch.cuda.synchronize()
        assert bool((out[M:] == -7.0).all()), "rows beyond M must not be written"
        outs[mask] = out
    assert torch.equal(outs[FC1_STORE].view(torch.int16), outs[0].view(torch.int16))
    # the plain twin is the kernel tests/test_gpu_kernels.py holds to torch; here only: it computed fc1, to half precision
    assert float((outs[0][:M].float() - want).norm() / want.norm()) < (1e-2 if dt == 0 else 2e-3)


# (M, N, K, rows per sample): tests/test_gated_rmw_shape.py
GATED_SHAPES = {
    "single_tile": (256, 192, 128, 256),
    "clamped_last_tile": (300, 192, 128, 300),
    "rolling_walk": (768, 1152, 192, 256),      # tiles walked across the rolling K pipeline: every A stage is refilled by hinted DMA
}


@pytest.mark.parametrize("dt", [0, 1], ids=["bf16", "f16"])
@pytest.mark.parametrize("name", list(GATED_SHAPES))
def test_gated_hinted_operand_equals_plain(lib, dev, policy, name, dt):
    """gemm_pwr_kernel<EPI_GATE_RES_F32, tag 0 / 1> (variant 11, epi 2): the A operand arrives in LDS by `nt` DMA -- same residual."""
    M, N, K, rps = GATED_SHAPES[name]
    Mp, A, W, bias = _operands(M, N, K, dt, dev, seed=M + N + K + 1)
    g = torch.Generator("cpu").manual_seed(M)
    gate = torch.randn((M + rps - 1) // rps, 2 * N, generator=g).to(dev)
    out0 = torch.randn(Mp, N, generator=g).to(dev)
    for tag, bit in ((0, PROJ_A), (1, FC2_A)):
        outs = {}
        for mask in (0, bit, ALL):
            policy(mask)
            out = out0.clone()
            check(lib.latte_debug_gemm(ptr(A), ptr(W), ptr(bias), ptr(out), ptr(gate), M, N, K, 2 * N, rps, 2, dt, 1000 * tag + 11, stream_ptr()))
            torch.cuda.synchronize()
            assert torch.equal(out[M:], out0[M:]), "rows beyond M must not be written"
            assert not torch.equal(out[:M], out0[:M])
            outs[mask] = out
        assert torch.equal(outs[bit], outs[0]), tag
        assert torch.equal(outs[ALL], outs[0]), tag


@pytest.mark.parametrize("dt", [0, 1], ids=["bf16", "f16"])
@pytest.mark.parametrize("mode", [0, 1], ids=["spatial", "temporal"])
def test_fused_attention_hinted_stores_equal_plain(lib, dev, policy, mode, dt):
    """qkv_attn_kernel<72, ...> with the default schedule (flags 7): the `nt` output stores write the same halves, all of them."""
    B, F, T, H, hd = 1, 16, 256, 8, 72          # tests/test_gpu_kernels.py FUSED_CASES: the smallest fusable shape at head_dim 72
    D, rows = H * hd, B * F * T
    g = torch.Generator("cpu").manual_seed(rows + hd + mode)
    xn = torch.randn(rows, D, generator=g).to(dev).to(TD[dt])
    W = (torch.randn(3 * D, D, generator=g) * D ** -0.5).to(dev).to(TD[dt])
    bias = (torch.randn(3 * D, generator=g) * 0.1).to(dev)
    outs = {}
    for mask in (0, ATTN_STORE):
        policy(mask)
        out = torch.full((rows, D), float("nan"), dtype=TD[dt], device=dev)
        check(lib.latte_debug_qkv_attention(ptr(xn), ptr(W), ptr(bias), ptr(out), None, B, F, T, D, H, mode, 7, dt, stream_ptr()))
        torch.cuda.synchronize()
        assert torch.isfinite(out).all()
        outs[mask] = out
    assert torch.equal(outs[ATTN_STORE].view(torch.int16), outs[0].view(torch.int16))


def test_debug_choice_refuses_other_values(lib):
    assert lib.latte_debug_set_choice(b"stream_policy", 5) != 0       # a mask without the 16
    assert lib.latte_debug_set_choice(b"stream_policy", 32) != 0
    check(lib.latte_debug_set_choice(b"stream_policy", 0))


@pytest.mark.parametrize("cd", ["f16", "bf16"])
def test_whole_model_and_option_round_trip(cd):
    """Depth 2, 256 tokens x 2 frames (tests/test_gated_rmw_shape.py), with fc1, the out-projection and fc2 on the kernels that have the
    hinted forms (the small shape would otherwise take other tiles): stream_policy 0 against 15, fc2 + temporal embedding included."""
    kw = dict(input_size=32, depth=2, hidden_size=1152, num_heads=16, num_frames=2, extras=1)
    torch.manual_seed(0)
    m = latte_amd.Latte(compute_dtype=cd, max_batch=2, **kw)
    g = torch.Generator("cpu").manual_seed(1)
    with torch.no_grad():
        for _, prm in m.named_parameters():     # the zero-initialised adaLN / final layer: non-zero gates
            if prm.requires_grad and float(prm.detach().abs().max()) == 0.0:
                prm.copy_(torch.randn(prm.shape, generator=g) * 0.5)
    m = m.cuda().eval()
    x = torch.randn(2, 2, 4, 32, 32, generator=g).cuda()
    t = torch.tensor([999, 12]).cuda()
    m.set_engine_option("gemm_variant_fc1", 9, 2)
    m.set_engine_option("gemm_variant_proj", 11, 2)
    m.set_engine_option("gemm_variant_fc2", 11, 2)
    assert 0 <= m.get_engine_option("stream_policy", 2) <= ALL   # the library's default
    outs = {}
    for mask in (0, ALL, 5):
        m.set_engine_option("stream_policy", mask, 2)
        assert m.get_engine_option("stream_policy", 2) == mask
        with torch.no_grad():
            outs[mask] = m(x, t).clone()
        torch.cuda.synchronize()
    assert torch.isfinite(outs[ALL]).all()
    assert torch.equal(outs[ALL], outs[0])
    assert torch.equal(outs[5], outs[0])
    with pytest.raises(Exception):
        m.set_engine_option("stream_policy", 16, 2)
