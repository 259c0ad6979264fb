"""The VAE engines' launch sequence, per kernel class, for three split-operand masks (csrc/vae_engine.cpp: vae_split_mask).

Which launches a decode / encode issues is decided by host code alone, so the per-class launch counts of latte_vae_profile_decode /
latte_vae_profile_encode are integers that a host refactor must reproduce exactly: tests/golden/vae_launch_counts.json holds them for
the smallest engines the creators accept (latent 16 / image 128), random weights."""
import ctypes
import json
import os

import pytest
import torch

from latte_amd._lib import check, ptr, stream_ptr

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vae_launch_counts.json")
ENGINES = ("spatial_decoder", "temporal_decoder", "encoder")
# latte_debug_set_choice("vae_split", value): 0 = the engine's default mask, (1 << 24) | m = the pass mask m
MASKS = {"default": 0, "all_off": (1 << 24) | 0, "all_on": (1 << 24) | 0xffffff}


def make_engine(name):
    """(engine object, input) of one case: weights from latte_amd/random_init.py (seed 0), a fixed input draw."""
    import latte_amd
    from latte_amd import random_init as ri
    g = torch.Generator("cpu").manual_seed(7)
    if name == "spatial_decoder":
        vae = latte_amd.AutoencoderKL(latent_size=16, max_frames=2)
        vae.load_state_dict(ri.vae_decoder_state_dict(0))
        x = torch.randn(2, 4, 16, 16, generator=g)
    elif name == "temporal_decoder":
        vae = latte_amd.AutoencoderKLTemporalDecoder(latent_size=16, max_frames=3)
        vae.load_state_dict(ri.vae_temporal_decoder_state_dict(0))
        x = torch.randn(3, 4, 16, 16, generator=g)
    else:
        vae = latte_amd.AutoencoderKL(max_frames=2, with_encoder=True)
        vae.load_state_dict(ri.vae_encoder_state_dict(0))
        x = torch.rand(2, 3, 128, 128, generator=g) * 2 - 1
    vae.to("cuda")
    return vae, x.cuda().contiguous()


def run_profiled(lib, name, vae, x):
    """One profiled call (out_mode 0) -> ({class: launches}, the output tensor)."""
    n = x.shape[0]
    k = len(vae.KERNEL_CLASSES)
    ms, cnt = (ctypes.c_float * k)(), (ctypes.c_int * k)()
    if name == "encoder":
        out = torch.empty(n, 8, 16, 16, device=x.device, dtype=torch.float32)
        check(lib.latte_vae_profile_encode(vae._enc_engine(128), ptr(x), n, 0, ptr(None), 1.0, 0, ptr(out), ms, cnt, k, stream_ptr()))
    else:
        out = torch.empty(n, 3, 128, 128, device=x.device, dtype=torch.float32)
        check(lib.latte_vae_profile_decode(vae._engine(n, 16), ptr(x), n, 1.0, 0, ptr(out), ms, cnt, k, stream_ptr()))
    return {c: int(cnt[i]) for i, c in enumerate(vae.KERNEL_CLASSES)}, out


@pytest.fixture(scope="module")
def engines():
    return {name: make_engine(name) for name in ENGINES}


@pytest.fixture
def kernel_choice(lib):
    """latte_debug_set_choice for the duration of a test."""
    used = []

    def choose(name, value):
        check(lib.latte_debug_set_choice(name.encode(), int(value)))
        used.append(name)
    yield choose
    for name in used:
        check(lib.latte_debug_set_choice(name.encode(), 0))


@pytest.mark.parametrize("mask", list(MASKS))
@pytest.mark.parametrize("name", ENGINES)
def test_vae_launch_counts(lib, engines, kernel_choice, name, mask):
    with open(GOLDEN) as f:
        want = json.load(f)[name][mask]
    vae, x = engines[name]
    kernel_choice("vae_split", MASKS[mask])
    got, out = run_profiled(lib, name, vae, x)
    print(name, mask, got)
    assert got == want
    assert set(got) == set(vae.KERNEL_CLASSES) and sum(got.values()) > 0
    assert bool(torch.isfinite(out).all())
