"""The gated GEMMs' fp32 read-modify-write epilogue  x += gate * (A W^T + bias)  of the rolling 12-wave kernel (gemm_pw.hip) in its two
residual access shapes -- fragment-wise (16 rows x 64 B per instruction) and line-wise (the whole 128-byte line of a wave's span as
8 rows x 128 B after a lane exchange) -- and the temporal embedding folded into the first block's fc2 epilogue.  Both are
re-arrangements of the same fp32 operations: every comparison between the forms is bit for bit."""
import pytest
import torch

import latte_amd
from latte_amd._lib import check, ptr, stream_ptr

pytestmark = pytest.mark.gpu
TD = {0: torch.bfloat16, 1: torch.float16}
GATED_TOL = 2e-5   # tests/test_gpu_kernels.py: the bound of this epilogue (epi 2) against torch on the same rounded operands
FRAGMENT_WISE, LINE_WISE = 1, 2   # latte_debug_set_choice("gated_rmw_shape", ...); 0 = the library's default


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda")


@pytest.fixture
def rmw_shape(lib):
    def choose(value):
        check(lib.latte_debug_set_choice(b"gated_rmw_shape", int(value)))
    yield choose
    check(lib.latte_debug_set_choice(b"gated_rmw_shape", 0))


def _operands(M, N, K, rps, dt, dev, seed):
    g = torch.Generator("cpu").manual_seed(seed)
    Mp = (M + 255) // 256 * 256 + 256          # one whole tile of padding rows behind the last (partial) tile
    A = torch.randn(Mp, K, generator=g).to(dev).to(TD[dt])
    W = (torch.randn(N, K, generator=g) / K ** 0.5).to(dev).to(TD[dt])
    bias = torch.randn(N, generator=g).to(dev)
    gate = torch.randn((M + rps - 1) // rps, 2 * N, generator=g).to(dev)
    out0 = torch.randn(Mp, N, generator=g).to(dev)   # the residual, N(0, 1)
    return A, W, bias, gate, out0


# (M, N, K, rows per sample)
SHAPES = {
    "single_tile": (256, 192, 128, 256),        # the smallest shape the kernel takes
    "shared_line": (256, 384, 128, 256),        # two tile columns: the line shared between wave spans and between tiles
    "clamped_last_tile": (300, 192, 128, 300),  # clamped last row tile; rows per sample % 256 != 0: the per-row path
    "clamped_fast_path": (600, 192, 128, 256),  # the clamped last row tile on the whole-tile-per-sample path (rows 512-599 of 768)
    "rolling_walk": (768, 1152, 192, 256),      # three samples with their own gate rows, tiles walked across the rolling K pipeline
}


@pytest.mark.parametrize("dt", [0, 1], ids=["bf16", "f16"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_line_wise_equals_fragment_wise(lib, dev, rmw_shape, name, dt):
    M, N, K, rps = SHAPES[name]
    A, W, bias, gate, out0 = _operands(M, N, K, rps, dt, dev, seed=M + N + K)
    smp = torch.arange(M, device=dev) // rps
    want = out0.double()[:M] + gate.double()[smp, :N] * (A.double()[:M] @ W.double().t() + bias.double())
    outs = {}
    for shape in (FRAGMENT_WISE, LINE_WISE):
        for tag in (0, 1):                      # out-projection / fc2 instantiation
            rmw_shape(shape)
            out = out0.clone()
            check(lib.latte_debug_gemm(ptr(A), ptr(W), ptr(bias), ptr(out), ptr(gate), M, N, K, 2 * N, rps, 2, dt, 1000 * tag + 11, stream_ptr()))
            torch.cuda.synchronize()
            rel = float((out.double()[:M] - want).norm() / want.norm())
            print(name, TD[dt], "shape", shape, "tag", tag, "rel", rel)
            assert rel < GATED_TOL, (shape, tag, rel)
            assert torch.equal(out[M:], out0[M:]), "rows beyond M must not be written"
            outs[shape, tag] = out
    for tag in (0, 1):
        assert torch.equal(outs[LINE_WISE, tag], outs[FRAGMENT_WISE, tag])
    assert torch.equal(outs[LINE_WISE, 0], outs[LINE_WISE, 1])


def test_line_wise_equals_fragment_wise_with_fp8_correction_pass(lib, dev, rmw_shape):
    """The correction-pass instantiation (GemmArgs::A8 / W8) shares the epilogue."""
    M, N, K, rps = 256, 192, 128, 256
    A, W, bias, gate, out0 = _operands(M, N, K, rps, 1, dev, seed=8)
    g = torch.Generator("cpu").manual_seed(9)

    def codes(shape):   # finite e4m3 codes below 16 in magnitude (tests/test_lo8.py)
        c = torch.randint(0, 256, shape, generator=g, dtype=torch.int32)
        c = torch.where((c & 0x7f) == 0x7f, c ^ 1, c)
        c = torch.where((c & 0x7f) > 0x57, c & 0xbf, c)
        return c.to(torch.uint8).to(dev)
    A8, W8 = codes(tuple(A.shape)), codes(tuple(W.shape))
    F8 = torch.float8_e4m3fn
    lo = (A8.view(F8).double()[:M] * 2.0 ** -12) @ (W8.view(F8).double() * 2.0 ** -6).t()
    want = out0.double()[:M] + gate.double()[:1, :N] * (A.double()[:M] @ W.double().t() + lo + bias.double())
    outs = {}
    for shape in (FRAGMENT_WISE, LINE_WISE):
        rmw_shape(shape)
        out = out0.clone()
        check(lib.latte_debug_gemm_lo8(ptr(A), ptr(W), ptr(A8), ptr(W8), ptr(bias), ptr(out), ptr(gate), M, N, K, 2 * N, rps, 2, 1, stream_ptr()))
        torch.cuda.synchronize()
        rel = float((out.double()[:M] - want).norm() / want.norm())
        print("fp8 correction, shape", shape, "rel", rel)
        assert rel < GATED_TOL, (shape, rel)
        assert torch.equal(out[M:], out0[M:])
        outs[shape] = out
    assert torch.equal(outs[LINE_WISE], outs[FRAGMENT_WISE])


@pytest.mark.parametrize("cd", ["f16", "bf16"])
@pytest.mark.parametrize("input_size", [8, 32], ids=["16_tokens", "256_tokens"])
def test_temp_embed_in_fc2_epilogue_keeps_the_bits(cd, input_size):
    """x + temp_embed after the first spatial block: added by that block's fc2 epilogue (engine option fc2_temp_embed = 1, fc2 on the
    rolling kernel) or by the next LayerNorm pass (= 0) -- the same two fp32 additions per element, identical outputs.  16 tokens x 2
    frames: 32 rows per sample, the epilogue's per-row path; 256 tokens: whole 256-row tiles per frame, its whole-tile path."""
    kw = dict(input_size=input_size, depth=2, hidden_size=1152, num_heads=16, num_frames=2, extras=1)
    torch.manual_seed(0)
    m = latte_amd.Latte(compute_dtype=cd, max_batch=2, **kw)
    g = torch.Generator("cpu").manual_seed(1)
    with torch.no_grad():
        for _, prm in m.named_parameters():     # the zero-initialised adaLN / final layer: non-zero gates
            if prm.requires_grad and float(prm.detach().abs().max()) == 0.0:
                prm.copy_(torch.randn(prm.shape, generator=g) * 0.5)
    assert float(m.temp_embed.abs().max()) > 0
    m = m.cuda().eval()
    x = torch.randn(2, 2, 4, input_size, input_size, generator=g).cuda()
    t = torch.tensor([999, 12]).cuda()
    outs = {}
    for fc2_variant in (11, 0):   # 11: fc2 on the rolling kernel (these small shapes otherwise take the 128 x 144 tile, which keeps the LayerNorm form)
        for fold in (0, 1):
            m.set_engine_option("gemm_variant_fc2", fc2_variant, 2)
            m.set_engine_option("fc2_temp_embed", fold, 2)
            assert m.get_engine_option("fc2_temp_embed", 2) == fold
            with torch.no_grad():
                outs[fc2_variant, fold] = m(x, t).clone()
            torch.cuda.synchronize()
    assert torch.isfinite(outs[11, 1]).all()
    assert torch.equal(outs[11, 1], outs[11, 0])
    assert torch.equal(outs[0, 1], outs[0, 0])
