"""SD-VAE decoder: oracle self-checks on CPU (parity with real diffusers is UNPINNED: oracle/vae_oracle.py),
host-shim behaviour, and — on the GPU — every VAE kernel and the whole decode against the oracle."""
import pytest
import torch
import torch.nn.functional as F

from _util import rel_l2
from oracle import vae_oracle as vo

TD = {0: torch.bfloat16, 1: torch.float16}
# north_star tolerance on the decoded frames: 1e-3 relative L2 against the fp32 restatement.  The decoder runs f16 MFMA
# operands (the reference decodes in fp16: sample.py:74, sample_t2x.py:32-34) on an fp32 residual stream; bf16 operands are
# not offered (7.3e-3 on the same decode: latte_amd/vae.py).
TOL = 1e-3


# ------------------------------------------------------------------------------------------------ CPU
def test_oracle_key_set_matches_diffusers_layout():
    ks = vo.decoder_keys()
    assert len(ks) == 140
    assert ks["decoder.conv_in.weight"] == (512, 4, 3, 3)
    assert ks["decoder.up_blocks.2.resnets.0.conv_shortcut.weight"] == (256, 512, 1, 1)
    assert ks["decoder.up_blocks.3.resnets.0.conv_shortcut.weight"] == (128, 256, 1, 1)
    assert "decoder.up_blocks.3.upsamplers.0.conv.weight" not in ks
    assert ks["decoder.mid_block.attentions.0.to_out.0.weight"] == (512, 512)
    assert sum(int(torch.tensor(s).prod()) for s in ks.values()) == 49_490_199   # decoder + post_quant parameters


def test_oracle_shapes_and_determinism():
    sd = vo.init_state_dict(seed=3)
    z = torch.randn(1, 4, 8, 8, generator=torch.Generator().manual_seed(0))
    a, b = vo.decode(sd, z), vo.decode(sd, z)
    assert a.shape == (1, 3, 64, 64) and torch.equal(a, b) and torch.isfinite(a).all()
    u8 = vo.to_uint8_video(a)
    assert u8.dtype == torch.uint8 and u8.shape == (1, 64, 64, 3)


def test_engine_key_set_equals_oracle_key_set(lib):
    import ctypes
    h = ctypes.c_void_p()
    # creating a VAE engine allocates device memory -> only the key enumeration of a failed create is host-only;
    # compare against the binding's expectation instead: every oracle key must be a slot the loader asks for.
    from latte_amd.vae import AutoencoderKL
    vae = AutoencoderKL()
    vae.load_state_dict({**vo.init_state_dict(0), "encoder.conv_in.weight": torch.zeros(1), "quant_conv.bias": torch.zeros(1)})
    assert set(vae.state_dict()) == set(vo.decoder_keys())
    legacy = {k.replace("to_q", "query").replace("to_k", "key").replace("to_v", "value").replace("to_out.0", "proj_attn"): v
              for k, v in vo.init_state_dict(0).items()}
    vae.load_state_dict(legacy)
    assert set(vae.state_dict()) == set(vo.decoder_keys())
    with pytest.raises(Exception):
        vae.decode(torch.zeros(1, 4, 16, 16))            # no GPU / not moved to cuda: must raise, never fall back
    with pytest.raises(Exception):
        vae.encode(torch.zeros(1, 3, 128, 128))
    with pytest.raises(Exception):
        AutoencoderKL(compute_dtype="bf16")              # f16 operands only (latte_amd/vae.py)
    with pytest.raises(Exception):
        vae.to(torch.bfloat16)
    assert vae.to(dtype=torch.float16).compute_dtype == "f16"     # the reference's own call (sample.py:74)


# ------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("dt", [1])
@pytest.mark.parametrize("kernel", [1, 3, 4], ids=["plain128", "pingpong256", "persistent256"])
@pytest.mark.parametrize("case", [(2, 16, 16, 64, 128, 0, False), (1, 16, 16, 128, 256, 1, False), (1, 8, 24, 256, 128, 0, True),
                                  (3, 5, 7, 64, 128, 1, True), (2, 32, 32, 512, 512, 0, True), (1, 32, 32, 256, 256, 1, False),
                                  (5, 128, 128, 128, 128, 0, True), (3, 64, 64, 256, 256, 1, False)])   # > 256 tiles: several per workgroup
def test_conv3x3_kernel(lib, dt, case, kernel):
    """Both implicit-GEMM kernels (csrc/vae.hip: the plain 128 x 128 tile and the round-4 ping-pong 256-pixel tile; the launcher
    picks by tile count, latte_debug_set_choice("conv_kernel", ...) forces one) against torch's conv2d on the same half operands:
    zero padding, nearest-2x upsample in the gather, partial last tile, half and fp32-stream epilogues."""
    from latte_amd._lib import check, ptr, stream_ptr
    check(lib.latte_debug_set_choice(b"conv_kernel", kernel))
    try:
        _conv3x3_case(lib, dt, case)
    finally:
        check(lib.latte_debug_set_choice(b"conv_kernel", 0))


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", [1, 3, 4], ids=["plain128", "pingpong256", "persistent256"])
@pytest.mark.parametrize("case", [(3, 70016, 64, 128), (14, 4096, 128, 256)])
def test_conv3_rows_kernel_wide_images(lib, kernel, case):
    """The 3-tap form (AutoencoderKLTemporalDecoder's Conv3d (3,1,1): frames are the rows of an "image" whose width is the frame's
    pixel count) at a width beyond 16 bits -- a 512 x 512 frame has 262 144 pixels -- and at a chunk of 14 frames."""
    from latte_amd._lib import check, ptr, stream_ptr
    T, HW, Cin, Cout = case
    dev = torch.device("cuda")
    g = torch.Generator("cpu").manual_seed(T + HW)
    x = torch.randn(T, HW, Cin, generator=g).half().to(dev)
    w = (torch.randn(Cout, 3, Cin, generator=g) / (3 * Cin) ** 0.5).half().to(dev)          # [co][ky][ci] = the packed layout
    b = torch.randn(Cout, generator=g).to(dev)
    r32 = torch.randn(T, HW, Cout, generator=g).to(dev)
    xp = torch.nn.functional.pad(x.float(), (0, 0, 0, 0, 1, 1))                                # zero frames before and after
    want = r32 + b + sum(xp[ky:ky + T] @ w[:, ky].float().t() for ky in range(3))
    out = torch.zeros(T, HW, Cout, device=dev)
    check(lib.latte_debug_set_choice(b"conv_kernel", kernel))
    try:
        check(lib.latte_debug_conv3rows_f32(ptr(x), ptr(w.reshape(Cout, 3 * Cin).contiguous()), ptr(b), ptr(r32), ptr(out), T, HW, Cin, Cout, 1,
                                            stream_ptr()))
    finally:
        check(lib.latte_debug_set_choice(b"conv_kernel", 0))
    torch.cuda.synchronize()
    assert rel_l2(out.cpu(), want.cpu()) < 2e-5


@pytest.mark.gpu
@pytest.mark.parametrize("case", [(5, 128, 128, 128, 128, 0), (2, 64, 64, 256, 256, 1), (6, 64, 64, 512, 256, 0)])
def test_persistent_conv_is_the_pingpong_conv_bit_for_bit(lib, case):
    """Round 6: conv3x3_pps_kernel walks several output tiles per workgroup with the gather two K tiles ahead across tile boundaries; same
    products in the same order as conv3x3_pp_kernel -> identical fp32 outputs (320 / 512 / 192 tiles: more and fewer than one per CU)."""
    from latte_amd._lib import check, ptr, stream_ptr
    N, H, W, Cin, Cout, ups = case
    dev = torch.device("cuda")
    g = torch.Generator("cpu").manual_seed(N * H + Cin)
    x = torch.randn(N, H, W, Cin, generator=g).half().to(dev)
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) / (3 * Cin ** 0.5)).to(dev)
    b = torch.randn(Cout, generator=g).to(dev)
    r32 = torch.randn(N, H << ups, W << ups, Cout, generator=g).to(dev)
    outs = {}
    for kernel in (3, 4):
        out = torch.zeros(N, H << ups, W << ups, Cout, device=dev)
        check(lib.latte_debug_set_choice(b"conv_kernel", kernel))
        try:
            check(lib.latte_debug_conv3x3_f32(ptr(x), ptr(w), ptr(b), ptr(r32), ptr(out), N, H, W, Cin, Cout, ups, 1, stream_ptr()))
        finally:
            check(lib.latte_debug_set_choice(b"conv_kernel", 0))
        torch.cuda.synchronize()
        outs[kernel] = out
    assert torch.equal(outs[3], outs[4])


def _conv3x3_case(lib, dt, case):
    from latte_amd._lib import check, ptr, stream_ptr
    N, H, W, Cin, Cout, ups, use_res = case
    g = torch.Generator("cpu").manual_seed(H * W + Cin)
    x = torch.randn(N, Cin, H, W, generator=g).to(TD[dt])
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / (3 * Cin ** 0.5)
    b = torch.randn(Cout, generator=g)
    Ho, Wo = H << ups, W << ups
    res = torch.randn(N, Cout, Ho, Wo, generator=g).to(TD[dt]) if use_res else None
    xin = x.float()
    if ups:
        xin = F.interpolate(xin, scale_factor=2.0, mode="nearest")
    want = F.conv2d(xin, w.to(TD[dt]).float(), b, padding=1)
    if use_res:
        want = want + res.float()
    dev = torch.device("cuda")
    xd = x.permute(0, 2, 3, 1).contiguous().to(dev)
    rd = res.permute(0, 2, 3, 1).contiguous().to(dev) if use_res else None
    out = torch.zeros(N, Ho, Wo, Cout, dtype=TD[dt], device=dev)
    wd, bd = w.to(dev), b.to(dev)        # keep the device copies alive across the (asynchronous) call
    check(lib.latte_debug_conv3x3(ptr(xd), ptr(wd), ptr(bd), ptr(rd), ptr(out), N, H, W, Cin, Cout, ups, dt,
                                  stream_ptr()))
    torch.cuda.synchronize()
    got = out.float().permute(0, 3, 1, 2).cpu()
    assert rel_l2(got, want) < (6e-3 if dt == 0 else 1e-3)
    # the decoder's fp32-stream form: fp32 residual in, fp32 out, nothing rounded after the accumulation
    r32 = torch.randn(N, Ho, Wo, Cout, generator=g).to(dev) if use_res else None
    out32 = torch.zeros(N, Ho, Wo, Cout, device=dev)
    check(lib.latte_debug_conv3x3_f32(ptr(xd), ptr(wd), ptr(bd), ptr(r32), ptr(out32), N, H, W, Cin, Cout, ups, dt,
                                      stream_ptr()))
    torch.cuda.synchronize()
    want32 = F.conv2d(xin, w.to(TD[dt]).float(), b, padding=1)
    if use_res:
        want32 = want32 + r32.cpu().permute(0, 3, 1, 2)
    assert rel_l2(out32.permute(0, 3, 1, 2).cpu(), want32) < 2e-5      # same rounded operands, fp32 accumulate


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [1])
@pytest.mark.parametrize("case", [(2, 256, 128, 1), (1, 1024, 512, 1), (1, 4096, 256, 0), (3, 100, 128, 1)])
def test_groupnorm_kernel(lib, dt, case):
    from latte_amd._lib import check, ptr, stream_ptr
    N, HW, C, silu = case
    g = torch.Generator("cpu").manual_seed(HW + C)
    x = (torch.randn(N, HW, C, generator=g) * 2 + 0.7).to(TD[dt])
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    want = F.group_norm(x.float().permute(0, 2, 1), 32, gamma, beta, 1e-6)
    if silu:
        want = F.silu(want)
    dev = torch.device("cuda")
    y = torch.zeros(N, HW, C, dtype=TD[dt], device=dev)
    xd, gd, bd = x.to(dev), gamma.to(dev), beta.to(dev)
    check(lib.latte_debug_groupnorm(ptr(xd), ptr(y), ptr(gd), ptr(bd), N, HW, C, silu, dt, stream_ptr()))
    torch.cuda.synchronize()
    assert rel_l2(y.float().permute(0, 2, 1).cpu(), want) < (5e-3 if dt == 0 else 8e-4)
    # fp32 input (the residual stream): only the output is rounded
    x32 = (torch.randn(N, HW, C, generator=g) * 2 + 0.7)
    want = F.group_norm(x32.permute(0, 2, 1), 32, gamma, beta, 1e-6)
    if silu:
        want = F.silu(want)
    xd32 = x32.to(dev)
    check(lib.latte_debug_groupnorm_f32(ptr(xd32), ptr(y), ptr(gd), ptr(bd), N, HW, C, silu, dt, stream_ptr()))
    torch.cuda.synchronize()
    assert rel_l2(y.float().permute(0, 2, 1).cpu(), want) < (3e-3 if dt == 0 else 4e-4)


@pytest.mark.gpu
@pytest.mark.parametrize("cd,tol", [("f16", TOL)])
def test_vae_decode_vs_oracle(lib, cd, tol):
    """Whole decoder on random weights, latent 16x16 -> 128x128, 2 frames (oracle: seconds on CPU)."""
    from latte_amd.vae import AutoencoderKL
    sd = vo.init_state_dict(seed=1)
    z = torch.randn(2, 4, 16, 16, generator=torch.Generator().manual_seed(5))
    want = vo.decode(sd, z)
    vae = AutoencoderKL(latent_size=16, max_frames=2, compute_dtype=cd)
    vae.load_state_dict(sd)
    vae.to("cuda")
    got = vae.decode(z.cuda()).sample
    torch.cuda.synchronize()
    assert got.shape == want.shape and torch.isfinite(got).all()
    err = rel_l2(got, want)
    print(f"vae decode [{cd}] rel-L2 vs oracle: {err:.3e}")
    assert err < tol
    # fused uint8 path = sample.py:122 applied to the fp32 result (one LSB of slack at rounding boundaries)
    lat = (z * 0.18215).view(1, 2, 4, 16, 16).cuda()
    u8 = vae.decode_video_uint8(lat)
    same_path = vae._run(lat.view(2, 4, 16, 16), 1.0 / 0.18215, 0)          # identical arithmetic, fp32 out
    ref8 = vo.to_uint8_video(same_path.cpu().clone())
    assert torch.equal(u8.view(2, 128, 128, 3).cpu(), ref8)
    # and against the oracle's own uint8 video: half-precision noise moves a few pixels by a few levels
    d = (u8.view(2, 128, 128, 3).cpu().int() - vo.to_uint8_video(want.clone()).int()).abs()
    print(f"uint8 video vs oracle: max level diff {int(d.max())}, mean {float(d.float().mean()):.3f}")
    assert float(d.float().mean()) < 0.3


@pytest.mark.gpu
@pytest.mark.parametrize("cd,tol", [("f16", TOL)])
def test_vae_stagewise_vs_oracle(lib, cd, tol):
    """Every traced decoder stage (conv_in, mid block, each up-block resnet / upsampler) against the oracle."""
    import ctypes
    from latte_amd._lib import check, ptr, stream_ptr
    from latte_amd.vae import AutoencoderKL
    sd = vo.init_state_dict(seed=2)
    z = torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(9))
    trace = []
    vo.decode(sd, z, trace=trace)
    assert len(trace) == 19
    vae = AutoencoderKL(latent_size=16, max_frames=1, compute_dtype=cd)
    vae.load_state_dict(sd)
    vae.to("cuda")
    zd = z.cuda()
    eng = vae._engine(1, 16)
    buf = torch.empty(1 * 128 * 128 * 256, device="cuda")
    numel, dims = ctypes.c_int64(), (ctypes.c_int * 4)()
    errs = []
    for k, want in enumerate(trace):
        check(lib.latte_debug_vae_trace(eng, ptr(zd), 1, 1.0, k, ptr(buf), ctypes.byref(numel), dims, stream_ptr()))
        torch.cuda.synchronize()
        n, h, w, c = list(dims)
        got = buf[:numel.value].view(n, h, w, c).permute(0, 3, 1, 2).cpu()
        assert got.shape == want.shape, (k, got.shape, want.shape)
        errs.append(rel_l2(got, want))
    print(f"vae stages [{cd}] rel-L2:", " ".join(f"{e:.1e}" for e in errs))
    assert max(errs) < tol, errs


ATTN = "decoder.mid_block.attentions.0."


def attention_inputs():
    """weights of vo.init_state_dict with to_v.bias and to_out.0.bias redrawn N(0, 1) (a missed bias fold is then as large as the
    contribution itself) and two frames of a 16 x 16 latent.  The four projection matrices are rounded to f16 values first: with
    unrounded ones the engine's f16 weight pack alone puts a correct engine at 2.3 x the yardstick below (CPU restatement with and
    without f16 weights: 1.69e-4 against 7.2e-5), which would say nothing about run_mid_attention; the weight pack is covered by the
    whole-decode tests."""
    sd = vo.init_state_dict(seed=12)
    g = torch.Generator().manual_seed(13)
    sd[ATTN + "to_v.bias"] = torch.randn(512, generator=g)
    sd[ATTN + "to_out.0.bias"] = torch.randn(512, generator=g)
    for k in ("to_q", "to_k", "to_v", "to_out.0"):     # f16-representable projection weights: the engine packs them to f16 at load, which
        sd[ATTN + k + ".weight"] = sd[ATTN + k + ".weight"].half().float()   # is then exact, so the six activation roundings are all there is
    return sd, torch.randn(2, 4, 16, 16, generator=g)


def attention_contribution(sd, x, half_roundings=False):
    """The mid-block attention's own contribution (its output before the residual is added) from the NHWC activation x [N, H, W, 512]:
    GroupNorm (eps 1e-6), one head of 512, softmax, out-projection, in x's precision.  half_roundings: round to f16 exactly where
    run_mid_attention (csrc/vae_engine.cpp) does -- the normed input, q, k, V0^T (the value bias is folded into the output bias
    there: to_out(P (V0 + 1 bv^T)) = to_out(P V0) + Wo bv + bo), P and the attention output."""
    r = (lambda t: t.half().to(t.dtype)) if half_roundings else (lambda t: t)
    w = lambda k: sd[ATTN + k].to(x.dtype)
    n, hh, ww, c = x.shape
    h = F.group_norm(x.permute(0, 3, 1, 2), 32, w("group_norm.weight"), w("group_norm.bias"), 1e-6)
    h = r(h.reshape(n, c, hh * ww).transpose(1, 2))
    q, k = r(F.linear(h, w("to_q.weight"), w("to_q.bias"))), r(F.linear(h, w("to_k.weight"), w("to_k.bias")))
    v0 = r(F.linear(h, w("to_v.weight")))
    p = r(torch.softmax(q @ k.transpose(1, 2) * (c ** -0.5), dim=-1))
    o = r(p @ v0)
    b_eff = w("to_out.0.weight") @ w("to_v.bias") + w("to_out.0.bias")
    return F.linear(o, w("to_out.0.weight"), b_eff).reshape(n, hh, ww, c)


def test_attention_contribution_restatement_is_the_oracle_attention():
    """the helper above, without roundings, is the oracle's attention minus its residual (so the bias fold it restates is right)"""
    sd, _ = attention_inputs()
    x = torch.randn(2, 16, 16, 512, generator=torch.Generator().manual_seed(1)).double()
    sd64 = {k: v.double() for k, v in sd.items()}
    want = vo._attention(sd64, ATTN, x.permute(0, 3, 1, 2)) - x.permute(0, 3, 1, 2)
    assert rel_l2(attention_contribution(sd, x).permute(0, 3, 1, 2), want) < 1e-12
    nobias = dict(sd)
    nobias[ATTN + "to_v.bias"] = torch.zeros(512)
    assert rel_l2(attention_contribution(nobias, x), attention_contribution(sd, x)) > 0.3     # a missed fold of the value bias is large


@pytest.mark.gpu
def test_vae_mid_attention_contribution(lib):
    """Stage 2 of the trace is the residual stream PLUS the attention's contribution, held to 1e-3 of the stream; here the contribution
    alone (stage 2 - stage 1) is compared with the fp64 attention of the engine's own stage-1 activation.  The tolerance is measured
    against a yardstick, not derived: a CPU restatement that rounds to f16 where run_mid_attention does has some relative L2 error
    against fp64; the engine must stay within twice that (summation order and the fast exponential are small next to six f16
    roundings).  Every frame's contribution must equal, bit for bit, that frame decoded alone."""
    import ctypes
    from latte_amd._lib import check, ptr, stream_ptr
    from latte_amd.vae import AutoencoderKL
    sd, z = attention_inputs()
    vae = AutoencoderKL(latent_size=16, max_frames=2, compute_dtype="f16")
    vae.load_state_dict(sd)
    vae.to("cuda")
    eng = vae._engine(2, 16)
    numel, dims = ctypes.c_int64(), (ctypes.c_int * 4)()

    def stage(zz, k):
        buf = torch.empty(zz.shape[0] * 16 * 16 * 512, device="cuda")
        check(lib.latte_debug_vae_trace(eng, ptr(zz), zz.shape[0], 1.0, k, ptr(buf), ctypes.byref(numel), dims, stream_ptr()))
        torch.cuda.synchronize()
        assert list(dims) == [zz.shape[0], 16, 16, 512] and numel.value == buf.numel()
        return buf.view(zz.shape[0], 16, 16, 512)
    zd = z.cuda()
    s1, s2 = stage(zd, 1), stage(zd, 2)
    got = (s2.double() - s1.double()).cpu()
    x = s1.cpu()
    want = attention_contribution(sd, x.double())
    yard = rel_l2(attention_contribution(sd, x, half_roundings=True).double(), want)
    err = rel_l2(got, want)
    print(f"mid attention contribution: engine rel-L2 vs fp64 {err:.3e}, f16-rounded CPU restatement {yard:.3e}, ratio {err / yard:.2f}; "
          f"|contribution| / |stream| {float(want.norm() / x.double().norm()):.3f}")
    assert err <= 2.0 * yard
    for f in range(2):
        a1, a2 = stage(zd[f:f + 1], 1), stage(zd[f:f + 1], 2)
        assert torch.equal(a1[0], s1[f]) and torch.equal(a2[0], s2[f])


@pytest.mark.gpu
def test_vae_full_size_decode_vs_oracle(lib):
    """The headline size: frames of a 32x32 latent -> 256x256 against the oracle (2 frames: ~10-20 s of CPU conv),
    default operand type, tolerance 1e-3."""
    from latte_amd.vae import AutoencoderKL
    sd = vo.init_state_dict(seed=6)
    z = torch.randn(2, 4, 32, 32, generator=torch.Generator().manual_seed(11))
    want = vo.decode(sd, z)
    vae = AutoencoderKL(latent_size=32, max_frames=2)
    vae.load_state_dict(sd)
    vae.to("cuda")
    got = vae.decode(z.cuda()).sample
    torch.cuda.synchronize()
    assert got.shape == want.shape == (2, 3, 256, 256) and torch.isfinite(got).all()
    err = rel_l2(got, want)
    print(f"vae decode 32x32 -> 256x256 [default dtype] rel-L2 vs oracle: {err:.3e}")
    assert err < TOL


@pytest.mark.gpu
def test_vae_full_size_frame_independence(lib):
    """Full reference size (16 frames of 32x32 latents -> 256x256): every frame of a batched decode equals the same frame
    decoded alone (GroupNorm statistics, attention and the implicit-GEMM tiles never mix frames) — a size-independent
    property checked where the CPU oracle would take minutes."""
    from latte_amd.vae import AutoencoderKL
    sd = vo.init_state_dict(seed=4)
    z = torch.randn(16, 4, 32, 32, generator=torch.Generator().manual_seed(2)).cuda()
    vae = AutoencoderKL(latent_size=32, max_frames=16, compute_dtype="f16")
    vae.load_state_dict(sd)
    vae.to("cuda")
    full = vae.decode(z).sample
    assert full.shape == (16, 3, 256, 256) and torch.isfinite(full).all() and float(full.std()) > 0
    for f in (0, 7, 15):
        one = vae.decode(z[f:f + 1]).sample
        assert torch.equal(one[0], full[f])


SD_SPLIT_MASKS = [0x0, 0xc00, 0x100c00, 0x301c00, 0x319c00, 0x319c03, 0x31bc07, 0xffffff & ~0x3e0]


@pytest.mark.gpu
def test_vae_split_mask_sweep(lib):
    """Round 6: the split-operand passes of csrc/vae_engine.cpp (vae_split_mask: activation / weight f16 rounding residuals per stage, the
    1x1 shortcuts, the upsampler convolutions, conv_out's input) on the SD-VAE decoder -- decode error against the fp32 restatement over
    five (weights, latent) draws and the time of a 16-frame 256 x 256 decode per mask.  RECORDED in gpurun_out/vae_split_sweep_sd.json
    (-> profiles/); asserted: the library's default mask holds the 1e-3 bar on every draw."""
    import json
    import os
    import time
    from _util import ROOT
    from latte_amd._lib import check
    from latte_amd.vae import AutoencoderKL
    draws = [(1, 2, 16, 5), (6, 2, 32, 11), (7, 1, 32, 3), (8, 2, 16, 4), (9, 1, 32, 6)]
    table = {f"{m:#08x}": {} for m in SD_SPLIT_MASKS}
    table["default"] = {}
    try:
        for seed, frames, latent, zseed in draws:
            sd = vo.init_state_dict(seed=seed)
            z = torch.randn(frames, 4, latent, latent, generator=torch.Generator().manual_seed(zseed))
            want = vo.decode(sd, z)
            vae = AutoencoderKL(latent_size=latent, max_frames=frames)
            vae.load_state_dict(sd)
            vae.to("cuda")
            for m in SD_SPLIT_MASKS + [None]:
                check(lib.latte_debug_set_choice(b"vae_split", 0 if m is None else (1 << 24) | m))
                got = vae.decode(z.cuda()).sample
                torch.cuda.synchronize()
                table["default" if m is None else f"{m:#08x}"][f"seed{seed}_{frames}x{latent}"] = rel_l2(got, want)
            del vae
        big = AutoencoderKL(latent_size=32, max_frames=16)
        big.load_state_dict(vo.init_state_dict(seed=4))
        big.to("cuda")
        zb = torch.randn(16, 4, 32, 32, generator=torch.Generator().manual_seed(1)).cuda()
        for m in SD_SPLIT_MASKS + [None]:
            check(lib.latte_debug_set_choice(b"vae_split", 0 if m is None else (1 << 24) | m))
            big.decode(zb)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(3):
                big.decode(zb)
            torch.cuda.synchronize()
            table["default" if m is None else f"{m:#08x}"]["ms_per_16_frame_decode"] = round((time.perf_counter() - t0) / 3 * 1e3, 2)
    finally:
        check(lib.latte_debug_set_choice(b"vae_split", 0))
    for k, row in table.items():
        errs = [v for kk, v in row.items() if kk.startswith("seed")]
        row["max"] = max(errs)
        print(k, f"max {row['max']:.3e}", " ".join(f"{e:.2e}" for e in errs), row["ms_per_16_frame_decode"], "ms")
    os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
    with open(os.path.join(ROOT, "gpurun_out", "vae_split_sweep_sd.json"), "w") as f:
        json.dump(table, f, indent=1)
    assert table["default"]["max"] < TOL
