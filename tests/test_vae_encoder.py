"""SD-VAE ENCODER (AutoencoderKL.encode, the reference's training-step call train.py:204-211): key layout, the fp32 restatement
(tests/vae_encoder_reference.py, parity with real diffusers UNPINNED), host-shim behaviour on CPU; on the GPU every new kernel, the
stage trace and the whole encode against the restatement, chunking, the uint8 path and the training driver on frame clips."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import vae_encoder_reference as er
from _util import rel_l2
from oracle import vae_oracle as vo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-3   # posterior mean and logvar, relative L2 against the fp32 restatement (f16 MFMA operands on an fp32 residual stream)


def _enc_sd(seed=0):
    from latte_amd.random_init import vae_encoder_state_dict
    return vae_encoder_state_dict(seed)


# ------------------------------------------------------------------------------------------------ CPU
def test_encoder_key_set_matches_diffusers_layout():
    from latte_amd.random_init import vae_encoder_keys
    ks = vae_encoder_keys()
    for i in range(4):
        for r in range(2):
            assert f"encoder.down_blocks.{i}.resnets.{r}.conv1.weight" in ks
        assert (f"encoder.down_blocks.{i}.downsamplers.0.conv.weight" in ks) == (i < 3)
    assert ks["encoder.down_blocks.0.downsamplers.0.conv.weight"] == (128, 128, 3, 3)
    assert ks["encoder.down_blocks.1.resnets.0.conv_shortcut.weight"] == (256, 128, 1, 1)
    assert ks["encoder.down_blocks.2.resnets.0.conv_shortcut.weight"] == (512, 256, 1, 1)
    assert [k for k in ks if "conv_shortcut.weight" in k] == ["encoder.down_blocks.1.resnets.0.conv_shortcut.weight",
                                                              "encoder.down_blocks.2.resnets.0.conv_shortcut.weight"]
    assert ks["encoder.mid_block.attentions.0.to_out.0.weight"] == (512, 512)
    assert ks["encoder.conv_in.weight"] == (128, 3, 3, 3)
    assert ks["encoder.conv_norm_out.weight"] == (512,)
    assert ks["encoder.conv_out.weight"] == (8, 512, 3, 3)
    assert ks["quant_conv.weight"] == (8, 8, 1, 1)
    # SD-VAE's 83,653,863 parameters minus the 49,490,199 of the decoder half (tests/test_vae.py)
    assert sum(math.prod(s) for s in ks.values()) == 34_163_664
    assert not set(ks) & set(vo.decoder_keys())


def test_reference_shapes_determinism_and_logvar_clamp():
    sd = _enc_sd(1)
    x = torch.rand(2, 3, 64, 48, generator=torch.Generator().manual_seed(0)) * 2 - 1
    trace = []
    a = er.encode_moments(sd, x, trace=trace)
    b = er.encode_moments(sd, x)
    assert a.shape == (2, 8, 8, 6) and torch.equal(a, b) and torch.isfinite(a).all()
    assert len(trace) == 16 and torch.equal(trace[-1], a)
    m = torch.zeros(1, 8, 2, 2)
    m[:, 4:] = torch.tensor([-100.0, 0.0, 100.0, 5.0]).view(1, 4, 1, 1)
    mean, logvar, std, var = er.posterior(m)
    assert logvar.flatten(1)[0, ::4].tolist() == [-30.0, 0.0, 20.0, 5.0]
    assert torch.allclose(std, torch.exp(0.5 * logvar)) and torch.allclose(var, torch.exp(logvar))


@pytest.mark.parametrize("hw", [(8, 8), (16, 12), (32, 32)])
def test_reference_downsample_is_pad_then_stride2(hw):
    g = torch.Generator().manual_seed(hw[0])
    x = torch.randn(2, 16, *hw, generator=g)
    w, b = torch.randn(16, 16, 3, 3, generator=g), torch.randn(16, generator=g)
    want = F.conv2d(F.pad(x, (0, 1, 0, 1)), w, b, stride=2)
    got = er.downsample(x, w, b)
    assert got.shape == (2, 16, hw[0] // 2, hw[1] // 2) and torch.equal(got, want)
    # output (y, x) reads input (2y + ky, 2x + kx); the bottom / right taps leave the image only at the last row / column
    y, xx = hw[0] // 2 - 1, hw[1] // 2 - 1
    patch = F.pad(x, (0, 1, 0, 1))[:, :, 2 * y:2 * y + 3, 2 * xx:2 * xx + 3]
    assert torch.allclose(got[:, :, y, xx], torch.einsum("nchw,ochw->no", patch, w) + b, atol=1e-4)


def test_host_shim_keeps_and_checks_encoder_keys(tmp_path):
    from latte_amd.vae import AutoencoderKL, LatteError
    from latte_amd.random_init import vae_decoder_state_dict, vae_encoder_keys
    full = {**vae_decoder_state_dict(0), **_enc_sd(0)}
    vae = AutoencoderKL(with_encoder=True)
    vae.load_state_dict(full)
    assert set(vae.state_dict()) == set(full)
    # legacy attention names (pre-0.18 diffusers) map as for the decoder, 1x1-conv shaped weights included
    legacy = {}
    for k, v in full.items():
        if ".attentions.0." in k and any(n in k for n in ("to_q", "to_k", "to_v", "to_out.0")):
            k = k.replace("to_q", "query").replace("to_k", "key").replace("to_v", "value").replace("to_out.0", "proj_attn")
            v = v.reshape(*v.shape, 1, 1) if v.dim() == 2 else v
        legacy[k] = v
    vae.load_state_dict(legacy)
    assert set(vae.state_dict()) == set(full)
    assert torch.equal(vae.state_dict()["encoder.mid_block.attentions.0.to_q.weight"], full["encoder.mid_block.attentions.0.to_q.weight"])
    with pytest.raises(LatteError, match="size mismatch"):
        vae.load_state_dict({**full, "encoder.conv_out.weight": torch.zeros(8, 512, 1, 1)})
    with pytest.raises(LatteError, match="Unexpected"):
        vae.load_state_dict({**full, "encoder.down_blocks.3.downsamplers.0.conv.weight": torch.zeros(512, 512, 3, 3)})
    # the default instance still drops the encoder half
    dec = AutoencoderKL()
    dec.load_state_dict(full)
    assert set(dec.state_dict()) == set(vo.decoder_keys())
    with pytest.raises(LatteError, match="with_encoder=True"):
        dec.encode(torch.zeros(1, 3, 128, 128))
    with pytest.raises(LatteError, match="with_encoder=True"):
        dec.encode_video_uint8(torch.zeros(1, 1, 128, 128, 3, dtype=torch.uint8))
    # with the encoder but on the CPU: raises, never falls back
    with pytest.raises(LatteError):
        vae.encode(torch.zeros(1, 3, 128, 128))
    # from_pretrained on a written diffusers directory passes with_encoder through
    from safetensors.torch import save_file
    d = tmp_path / "vae"
    d.mkdir()
    save_file({k: v.contiguous() for k, v in full.items()}, str(d / "diffusion_pytorch_model.safetensors"))
    (d / "config.json").write_text('{"scaling_factor": 0.18215, "block_out_channels": [128, 256, 512, 512]}')
    fp = AutoencoderKL.from_pretrained(str(tmp_path), subfolder="vae", with_encoder=True)
    assert fp.with_encoder and set(fp.state_dict()) == set(full)
    assert set(AutoencoderKL.from_pretrained(str(tmp_path), subfolder="vae").state_dict()) == set(vo.decoder_keys())
    assert set(vae_encoder_keys()) <= set(fp.state_dict())


def test_encode_clips_help():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "encode_clips.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--src" in r.stdout and "--dst" in r.stdout, r.stderr


# ------------------------------------------------------------------------------------------------ GPU
def _encoder(size, frames, seed=0, sd=None):
    from latte_amd.vae import AutoencoderKL
    vae = AutoencoderKL(max_frames=frames, with_encoder=True)
    vae.load_state_dict(sd if sd is not None else _enc_sd(seed))
    return vae.to("cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", [1, 3, 4], ids=["plain128", "pingpong256", "persistent256"])
@pytest.mark.parametrize("case", [(3, 256, 128), (3, 128, 256), (5, 64, 512)], ids=["128ch_256", "256ch_128", "512ch_64"])
def test_downsample_conv_kernel(lib, case, kernel):
    """The stride-2 gather of the implicit-GEMM convolution (Downsample2D: pad (0, 1, 0, 1), 3x3 stride 2) at the encoder's three
    shapes with an odd frame count, through each kernel form, against torch's conv2d of the padded input on the same f16 operands."""
    from latte_amd._lib import check, ptr, stream_ptr
    N, Hin, C = case
    dev = torch.device("cuda")
    g = torch.Generator("cpu").manual_seed(Hin + C)
    x = torch.randn(N, Hin, Hin, C, generator=g).half().to(dev)
    w = (torch.randn(C, C, 3, 3, generator=g) / (3 * C ** 0.5)).to(dev)
    b = torch.randn(C, generator=g).to(dev)
    r32 = torch.randn(N, Hin // 2, Hin // 2, C, generator=g).to(dev)
    want = F.conv2d(F.pad(x.float().permute(0, 3, 1, 2), (0, 1, 0, 1)), w.half().float(), b, stride=2).permute(0, 2, 3, 1) + r32
    out = torch.zeros(N, Hin // 2, Hin // 2, C, device=dev)
    check(lib.latte_debug_set_choice(b"conv_kernel", kernel))
    try:
        check(lib.latte_debug_conv3x3_down_f32(ptr(x), ptr(w), ptr(b), ptr(r32), ptr(out), N, Hin, Hin, C, C, 1, stream_ptr()))
    finally:
        check(lib.latte_debug_set_choice(b"conv_kernel", 0))
    torch.cuda.synchronize()
    assert rel_l2(out.cpu(), want.cpu()) < 1e-3


@pytest.mark.gpu
def test_encoder_conv_in_fp32_and_uint8(lib):
    from latte_amd._lib import check, ptr, stream_ptr
    dev = torch.device("cuda")
    g = torch.Generator("cpu").manual_seed(11)
    N, H, W = 3, 64, 48
    w, b = torch.randn(128, 3, 3, 3, generator=g).to(dev) / 5, torch.randn(128, generator=g).to(dev)
    u8 = torch.randint(0, 256, (N, H, W, 3), generator=g, dtype=torch.uint8).to(dev)
    xf = (u8.float() / 127.5 - 1).permute(0, 3, 1, 2).contiguous()
    want = F.conv2d(xf, w, b, padding=1).permute(0, 2, 3, 1)
    got32, got8 = torch.empty(N, H, W, 128, device=dev), torch.empty(N, H, W, 128, device=dev)
    check(lib.latte_debug_vae_enc_conv_in(ptr(xf), 0, ptr(w), ptr(b), ptr(got32), N, H, W, stream_ptr()))
    check(lib.latte_debug_vae_enc_conv_in(ptr(u8), 1, ptr(w), ptr(b), ptr(got8), N, H, W, stream_ptr()))
    torch.cuda.synchronize()
    assert rel_l2(got32.cpu(), want.cpu()) < 1e-6
    assert rel_l2(got8.cpu(), got32.cpu()) < 1e-6          # the uint8 path = the fp32 path on x / 127.5 - 1, to fp32 rounding


@pytest.mark.gpu
@pytest.mark.parametrize("split", [False, True])
def test_encoder_tail_moments_mode_sample(lib, split):
    """conv_out (512 -> 8) with quant_conv folded in, then the posterior, against torch on the same conv_out input."""
    from latte_amd._lib import check, ptr, stream_ptr
    dev = torch.device("cuda")
    g = torch.Generator("cpu").manual_seed(21)
    N, H, W = 3, 32, 16
    xs = torch.randn(N, H, W, 512, generator=g)
    hi = xs.half()
    lo = (xs - hi.float()).half()
    w, b = torch.randn(8, 512, 3, 3, generator=g) / 48, torch.randn(8, generator=g)
    qw, qb = torch.randn(8, 8, 1, 1, generator=g) / 3, torch.randn(8, generator=g)
    xin = (hi.float() + lo.float()) if split else hi.float()
    want = F.conv2d(F.conv2d(xin.permute(0, 3, 1, 2), w, b, padding=1), qw, qb)
    mom = torch.empty(N, 8, H, W, device=dev)
    hid, lod, wd, bd, qwd, qbd = (t.to(dev) for t in (hi, lo, w, b, qw, qb))        # held: the kernel reads them after ptr() returns
    check(lib.latte_debug_vae_enc_tail(ptr(hid), ptr(lod if split else None), ptr(wd), ptr(bd), ptr(qwd), ptr(qbd), ptr(mom), N, H, W,
                                       stream_ptr()))
    torch.cuda.synchronize()
    assert rel_l2(mom.cpu(), want) < 1e-5
    noise = torch.randn(N, 4, H, W, generator=g).to(dev)
    outs = {}
    for what in (1, 2, 3, 4, 5):
        o = torch.empty(N, 4, H, W, device=dev)
        check(lib.latte_vae_posterior(ptr(mom), ptr(noise), N, H * W, 0.18215, what, ptr(o), stream_ptr()))
        outs[what] = o
    torch.cuda.synchronize()
    mean, logvar, std, var = er.posterior(mom.cpu())
    assert rel_l2(outs[1].cpu(), mean * 0.18215) < 1e-6
    assert rel_l2(outs[2].cpu(), (mean + torch.exp(0.5 * torch.clamp(mom.cpu()[:, 4:], -30, 20)) * noise.cpu()) * 0.18215) < 1e-6
    assert rel_l2(outs[3].cpu(), logvar) < 1e-6 and rel_l2(outs[4].cpu(), std) < 1e-6 and rel_l2(outs[5].cpu(), var) < 1e-6


@pytest.mark.gpu
def test_encoder_stage_trace_vs_reference(lib):
    """Every traced encoder stage (conv_in, each down-block resnet / down-sampler, the mid block, the moments) against the restatement."""
    from latte_amd._lib import check, ptr, stream_ptr
    sd = _enc_sd(2)
    x = torch.rand(2, 3, 128, 128, generator=torch.Generator().manual_seed(9)) * 2 - 1
    trace = []
    er.encode_moments(sd, x, trace=trace)
    assert len(trace) == 16
    vae = _encoder(128, 2, sd=sd)
    eng = vae._enc_engine(128)
    xd = x.cuda().contiguous()
    buf = torch.empty(2 * 128 * 128 * 128, device="cuda")
    numel, dims = ctypes.c_int64(), (ctypes.c_int * 4)()
    errs = []
    for k, want in enumerate(trace):
        check(lib.latte_debug_vae_encode_trace(eng, ptr(xd), 2, 0, k, ptr(buf), ctypes.byref(numel), dims, stream_ptr()))
        torch.cuda.synchronize()
        d = list(dims)
        got = buf[:numel.value].view(*d)
        got = (got if k == 15 else got.permute(0, 3, 1, 2)).cpu()
        assert got.shape == want.shape, (k, got.shape, want.shape)
        errs.append(rel_l2(got, want))
    print("encoder stages rel-L2:", " ".join(f"{e:.1e}" for e in errs))
    assert max(errs) < TOL, errs
    with pytest.raises(Exception):
        check(lib.latte_debug_vae_encode_trace(eng, ptr(xd), 2, 0, 16, ptr(buf), ctypes.byref(numel), dims, stream_ptr()))


def _posterior_errors(vae, sd, x):
    d = vae.encode(x.cuda()).latent_dist
    want = er.encode_moments(sd, x)
    mean, logvar, _, _ = er.posterior(want)
    return rel_l2(d.mean.cpu(), mean), rel_l2(d.logvar.cpu(), logvar), d


@pytest.mark.gpu
def test_full_size_encode_vs_reference_five_draws(lib):
    """The training size: 16 frames of 256 x 256, five draws of input and random sd-vae-shaped weights; posterior mean and logvar each
    within 1e-3 relative L2 of the fp32 restatement."""
    errs = []
    for draw in range(5):
        sd = _enc_sd(100 + draw)
        x = torch.rand(16, 3, 256, 256, generator=torch.Generator().manual_seed(200 + draw)) * 2 - 1
        vae = _encoder(256, 16, sd=sd)
        em, el, d = _posterior_errors(vae, sd, x)
        assert d.parameters.shape == (16, 8, 32, 32) and torch.isfinite(d.parameters).all()
        errs.append((em, el))
        del vae
    print("encode 16 x 256^2 (mean, logvar) rel-L2:", " ".join(f"({a:.2e}, {b:.2e})" for a, b in errs))
    assert max(max(e) for e in errs) < TOL, errs


@pytest.mark.gpu
def test_encode_128_eight_frames_vs_reference(lib):
    sd = _enc_sd(7)
    x = torch.rand(8, 3, 128, 128, generator=torch.Generator().manual_seed(70)) * 2 - 1
    vae = _encoder(128, 8, sd=sd)
    em, el, d = _posterior_errors(vae, sd, x)
    assert d.parameters.shape == (8, 8, 16, 16)
    assert em < TOL and el < TOL, (em, el)


@pytest.mark.gpu
def test_encoder_handle_rejects_decode_and_bad_sizes(lib):
    from latte_amd._lib import c_void, check, ptr, stream_ptr
    vae = _encoder(128, 2)
    eng = vae._enc_engine(128)
    z = torch.zeros(1, 4, 16, 16, device="cuda")
    out = torch.empty(1, 3, 128, 128, device="cuda")
    assert lib.latte_vae_decode(eng, ptr(z), 1, 1.0, 0, ptr(out), stream_ptr()) == 1          # LATTE_ERR_INVALID
    assert b"encoder" in lib.latte_last_error()
    h = c_void()
    assert lib.latte_vae_create_encoder(200, 1, 1, ctypes.byref(h)) != 0
    assert b"image_size" in lib.latte_last_error()


@pytest.mark.gpu
def test_encode_chunking_is_per_chunk_bits(lib):
    """n_frames > max_frames: chunked by max_frames inside encode, the same bits as separate per-chunk calls."""
    vae = _encoder(128, 4, seed=3)
    x = (torch.rand(10, 3, 128, 128, generator=torch.Generator().manual_seed(30)) * 2 - 1).cuda()
    whole = vae.encode(x).latent_dist.parameters
    parts = torch.cat([vae.encode(x[s:s + 4]).latent_dist.parameters for s in range(0, 10, 4)])
    assert torch.equal(whole, parts)


@pytest.mark.gpu
def test_reference_line_equals_encode_video_uint8(lib):
    """`vae.encode(x).latent_dist.sample(generator=g).mul_(0.18215)` (train.py:210) on x = frames / 127.5 - 1 equals
    encode_video_uint8(frames) with the same generator, and .sample() is mean + std * noise of the returned moments."""
    vae = _encoder(128, 8, seed=4)
    g = torch.Generator("cpu").manual_seed(40)
    frames = torch.randint(0, 256, (2, 3, 128, 128, 3), generator=g, dtype=torch.uint8)
    x = (frames.float() / 127.5 - 1).reshape(6, 128, 128, 3).permute(0, 3, 1, 2).contiguous().cuda()
    dist = vae.encode(x).latent_dist
    ref = dist.sample(generator=torch.Generator("cuda").manual_seed(5)).mul_(0.18215)
    got = vae.encode_video_uint8(frames.cuda(), generator=torch.Generator("cuda").manual_seed(5))
    assert got.shape == (2, 3, 4, 16, 16)
    assert rel_l2(got.reshape(6, 4, 16, 16).cpu(), ref.cpu()) < 1e-5
    noise = torch.randn(6, 4, 16, 16, generator=torch.Generator("cuda").manual_seed(5), device="cuda")
    m = dist.parameters
    manual = m[:, :4] + torch.exp(0.5 * torch.clamp(m[:, 4:], -30, 20)) * noise
    assert rel_l2(dist.sample(generator=torch.Generator("cuda").manual_seed(5)).cpu(), manual.cpu()) < 1e-6
    assert torch.equal(dist.mode(), dist.mean) and dist.mean.data_ptr() == m.data_ptr()


@pytest.mark.gpu
def test_train_driver_on_uint8_frame_clips(tmp_path):
    """tools/train.py with data_path = uint8 frame clips: every batch encoded on the GPU (random-weight VAE directory), a few steps,
    finite losses, a checkpoint."""
    from safetensors.torch import save_file
    from latte_amd.random_init import vae_decoder_state_dict
    vdir = tmp_path / "pretrained" / "vae"
    vdir.mkdir(parents=True)
    save_file({k: v.contiguous() for k, v in {**vae_decoder_state_dict(0), **_enc_sd(0)}.items()},
              str(vdir / "diffusion_pytorch_model.safetensors"))
    data = tmp_path / "clips"
    data.mkdir()
    rng = np.random.default_rng(0)
    for i in range(3):
        np.save(data / f"{i % 5}_clip{i}.npy", rng.integers(0, 256, (4, 128, 128, 3), dtype=np.uint8))
    cfg = open(os.path.join(ROOT, "configs", "tiny_train.yaml")).read()
    cfg = cfg.replace('data_path: "synthetic"', f'data_path: "{data}"').replace("image_size: 64", "image_size: 128")
    cfg += f'pretrained_model_path: "{tmp_path / "pretrained"}"\n'
    (tmp_path / "cfg.yaml").write_text(cfg)
    out = str(tmp_path / "run")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "train.py"), "--config", str(tmp_path / "cfg.yaml"), "--out", out,
                        "--max-steps", "4", "--log-every", "2"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    losses = [float(l.split("Train Loss: ")[1].split(",")[0]) for l in r.stdout.splitlines() if "Train Loss" in l]
    assert len(losses) == 2 and all(math.isfinite(v) for v in losses), r.stdout
    assert os.path.exists(os.path.join(out, "checkpoints", "0000004.pt"))
