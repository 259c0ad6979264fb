"""Training from stored VAE moments on the GPU: ``latte_moment_sample`` (latte_amd/csrc/moments.hip) against
``latte_vae_posterior`` on the torch-gathered rows BIT FOR BIT -- both run the device function ``posterior_value`` --, its in-kernel
Philox draw against ``latte_debug_fill_normal``, its refusals; then ``latte_amd.MomentStore`` against the encoder it was built with, the
raw path's latents, the host-resident store, and the drivers (tools/encode_clips.py --moments, tools/train.py on ``moments_path``)."""
import ctypes
import math
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from _util import rel_l2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1
SCALE = 0.18215
N_ROWS = 37 * 2                    # 37 frames x 2 planes
SEED_NONE = 2 ** 64 - 1


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(None)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _store(hw, half, seed=0):
    """[N_ROWS, 8, hw]: N(0, 1) means, logvars wide enough to pass both clamps (-30 and 20)."""
    g = torch.Generator().manual_seed(seed)
    m = torch.randn(N_ROWS, 8, hw, generator=g)
    m[:, 4:] *= 25.0
    assert (m[:, 4:] < -30).any() and (m[:, 4:] > 20).any()
    m = m.cuda()
    return m.half() if half else m


def _rows(n):
    """Row 0, the last row, repeats and a descending run, cut / tiled to n entries (n == 1: the last row)."""
    base = [N_ROWS - 1, 0, 0, N_ROWS - 1, 5, 5] + list(range(N_ROWS - 1, -1, -1)) + [17, 3, 17]
    return np.array((base * (n // len(base) + 1))[:n], dtype=np.int64)


def _sample(lib, store, rows, what, noise=None, seed=0, offset=0, scale=SCALE, out=None, n_rows=None, hw=None):
    n, hw = len(rows), store.shape[2] if hw is None else hw
    if out is None:
        out = torch.full((n, 8 if what == 0 else 4, hw), -777.0, device="cuda")
    rc = lib.latte_moment_sample(_ptr(store), int(store.dtype == torch.float16), store.shape[0] if n_rows is None else n_rows, hw,
                                 rows.ctypes.data_as(ctypes.c_void_p), n, _ptr(noise), seed, offset, scale, what, _ptr(out), _stream())
    return rc, out


def _posterior(lib, gathered, noise, what):
    n, _, hw = gathered.shape
    out = torch.empty(n, 4, hw, device="cuda")
    assert lib.latte_vae_posterior(_ptr(gathered), _ptr(noise), n, hw, SCALE, what, _ptr(out), _stream()) == 0, lib.latte_last_error()
    return out


# ------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.gpu
@pytest.mark.parametrize("what", [0, 1, 2])
@pytest.mark.parametrize("hw", [8, 24, 256, 1024])
@pytest.mark.parametrize("half", [False, True], ids=["fp32", "f16"])
def test_kernel_equals_posterior_on_gathered_rows(lib, half, hw, what):
    store = _store(hw, half, seed=hw)
    for n in (1, 80, 257):                                    # 257 crosses the 256-row launch boundary
        rows = _rows(n)
        gathered = store.float()[torch.from_numpy(rows).cuda()].contiguous()
        noise = torch.randn(n, 4, hw, generator=torch.Generator().manual_seed(n)).cuda() if what == 2 else None
        rc, got = _sample(lib, store, rows, what, noise)
        assert rc == 0, lib.latte_last_error()
        want = gathered if what == 0 else _posterior(lib, gathered, noise, what)
        assert torch.isfinite(got).all() and torch.equal(got, want), (n, float((got - want).abs().max()))


@pytest.mark.gpu
@pytest.mark.parametrize("offset", [0, 4 * 123457 + 3, (1 << 33) + 8], ids=["0", "unaligned", "above_2_33"])
@pytest.mark.parametrize("half", [False, True], ids=["fp32", "f16"])
def test_inline_noise_is_the_generator_bit_for_bit(lib, half, offset):
    hw, n, seed = 24, 257, 20240611
    store, rows = _store(hw, half, seed=3), _rows(n)
    z = torch.empty(n, 4, hw, device="cuda")
    assert lib.latte_debug_fill_normal(_ptr(z), z.numel(), seed, offset, _stream()) == 0, lib.latte_last_error()
    rc1, given = _sample(lib, store, rows, 2, z)
    rc2, inline = _sample(lib, store, rows, 2, None, seed, offset)
    assert rc1 == 0 and rc2 == 0, lib.latte_last_error()
    assert torch.equal(inline, given)
    rc3, other = _sample(lib, store, rows, 2, None, seed + 1, offset)
    assert rc3 == 0 and not torch.equal(other, inline)


@pytest.mark.gpu
def test_refusals_leave_out_untouched(lib):
    hw = 24
    store = _store(hw, False)
    noise = torch.zeros(4, 4, hw, device="cuda")
    ok = np.array([0, 1, 2, 3], dtype=np.int64)
    sentinel = torch.full((4, 4, hw), -777.0, device="cuda")

    def refused(what_in_error, rows=ok, what=2, noise=noise, **kw):
        rc, _ = _sample(lib, store, rows, what, noise, out=sentinel, **kw)
        assert rc == INVALID and what_in_error in lib.latte_last_error(), (rc, lib.latte_last_error())
        torch.cuda.synchronize()
        assert bool((sentinel == -777.0).all())

    refused(b"rows[2] = -1", rows=np.array([0, 1, -1, 3], dtype=np.int64))
    refused(b"rows[3] = 74", rows=np.array([0, 1, 2, N_ROWS], dtype=np.int64))
    refused(b"rows[0] = 74", rows=np.array([N_ROWS], dtype=np.int64), what=0)
    refused(b"multiple of 8", hw=12)
    refused(b"moment_sample", rows=np.array([], dtype=np.int64))             # n_out = 0
    refused(b"bad shape", n_rows=0)
    refused(b"what must be", what=3)
    refused(b"noise or a seed", noise=None, seed=SEED_NONE)                  # what = 2 with neither noise nor a seed
    # null pointers (store, rows, out), called directly
    for args in ((None, ok.ctypes.data_as(ctypes.c_void_p), _ptr(sentinel)), (_ptr(store), None, _ptr(sentinel)),
                 (_ptr(store), ok.ctypes.data_as(ctypes.c_void_p), None)):
        assert lib.latte_moment_sample(args[0], 0, N_ROWS, hw, args[1], 4, _ptr(noise), 0, 0, SCALE, 2, args[2], _stream()) == INVALID
        assert b"null argument" in lib.latte_last_error()
    torch.cuda.synchronize()
    assert bool((sentinel == -777.0).all())


# ------------------------------------------------------------------------------------------------ the store against the encoder
NUM_FRAMES, INTERVAL = 4, 2


@pytest.fixture(scope="module")
def enc(lib):
    """The random-weight encoder at 128 x 128 with max_frames 4, two raw clips, and the stores of both UCF-style pipelines."""
    import latte_amd
    from latte_amd import video_transforms
    from latte_amd.random_init import vae_encoder_state_dict
    vae = latte_amd.AutoencoderKL(max_frames=4, with_encoder=True)
    vae.load_state_dict(vae_encoder_state_dict(0))
    vae.to("cuda")
    g = torch.Generator().manual_seed(11)
    clips = [("3_small", torch.randint(0, 256, (9, 36, 48, 3), generator=g, dtype=torch.uint8)),
             ("1_square", torch.randint(0, 256, (6, 128, 128, 3), generator=g, dtype=torch.uint8))]
    transforms = {d: video_transforms.get_transform(SimpleNamespace(dataset=d, num_frames=NUM_FRAMES, frame_interval=INTERVAL, image_size=128))[0]
                  for d in ("ucf101", "ffs")}
    # e: how much a frame's moments depend on the chunk it is encoded in, on code that existed before the store
    x = transforms["ucf101"](clips[0][1][:4].cuda())
    chunk = vae.encode(x).latent_dist.parameters
    alone = torch.cat([vae.encode(x[i:i + 1]).latent_dist.parameters for i in range(4)])
    e = float((chunk - alone).abs().max())
    print(f"frame alone vs inside a four-frame chunk: max abs difference e = {e:.3e}")
    stores = {(d, dt): latte_amd.MomentStore.build(vae, clips, t, dtype=dt).to("cuda") for d, t in transforms.items() for dt in ("fp32", "f16")}
    return SimpleNamespace(vae=vae, clips=clips, transforms=transforms, stores=stores, e=e)


@pytest.mark.gpu
@pytest.mark.parametrize("dataset", ["ucf101", "ffs"])
def test_stored_moments_are_the_encoders(enc, dataset):
    store, t = enc.stores[(dataset, "fp32")], enc.transforms[dataset]
    assert store.planes == (False, True) and store.clip_frames == [9, 6] and store.labels == [3, 1] and store.latent_hw == (16, 16)
    assert store.dtype == "fp32" and store.nbytes == 15 * 2 * 8 * 256 * 4
    worst = 0.0
    for c, (_, frames) in enumerate(enc.clips):
        for j in range(frames.shape[0]):
            for plane in (False, True):
                alone = enc.vae.encode_video_raw_moments(frames[j:j + 1], t, flip=[plane])[0, 0]
                got = store.moments(store.frame_rows(c, [j], plane))[0]
                if enc.e == 0:
                    assert torch.equal(got, alone), (c, j, plane)
                worst = max(worst, float((got - alone).abs().max()))
    print(f"stored vs alone: max abs difference {worst:.3e} (bound e = {enc.e:.3e})")
    assert worst <= enc.e
    # the planes differ, and f16 storage is the rounded fp32 store, nothing else
    both = store.moments(np.arange(store.num_rows)).view(15, 2, 8, 16, 16)
    assert not torch.equal(both[:, 0], both[:, 1])
    half = enc.stores[(dataset, "f16")]
    assert half.dtype == "f16" and half.nbytes * 2 == store.nbytes and torch.equal(half._data, store._data.half())


@pytest.mark.gpu
@pytest.mark.parametrize("clip,start,flip,interval", [(0, 0, False, 2), (0, 1, True, 2), (1, 2, True, 1)])
def test_same_latents_as_the_raw_path(enc, clip, start, flip, interval):
    from latte_amd.video_transforms import frame_indices
    store, t = enc.stores[("ucf101", "fp32")], enc.transforms["ucf101"]
    idx = frame_indices(start, start + NUM_FRAMES * interval, NUM_FRAMES)
    got = store.sample_clips([clip], [start], [flip], NUM_FRAMES, interval, generator=torch.Generator("cuda").manual_seed(77))
    want = enc.vae.encode_video_raw(enc.clips[clip][1][idx].cuda(), t, flip=[flip], generator=torch.Generator("cuda").manual_seed(77))
    assert got.shape == want.shape == (1, NUM_FRAMES, 4, 16, 16)
    err = rel_l2(got.cpu(), want.cpu())
    print(f"sample_clips vs encode_video_raw (clip {clip}, start {start}, flip {flip}): rel L2 {err:.3e}")
    assert err < 1e-5
    other = store.sample_clips([clip], [start], [not flip], NUM_FRAMES, interval, generator=torch.Generator("cuda").manual_seed(77))
    assert not torch.equal(other, got)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["fp32", "f16"])
def test_host_resident_store_gives_the_same_bits(enc, tmp_path, dtype):
    import latte_amd
    enc.stores[("ffs", dtype)].save(str(tmp_path))
    dev, host = latte_amd.MomentStore.load(str(tmp_path), device="cuda"), latte_amd.MomentStore.load(str(tmp_path), device="cpu")
    assert dev.device.type == "cuda" and host.device.type == "cpu" and dev.names == host.names == ["1_square", "3_small"]
    assert torch.equal(dev._data.cpu(), host._data) and host.dtype == dev.dtype == dtype
    clips, starts, flips = [1, 0, 1], [0, 0, 1], [True, False, False]
    for kw in (dict(seed=5), dict(noise=torch.randn(12, 4, 16, 16, generator=torch.Generator().manual_seed(1)).cuda())):
        assert torch.equal(dev.sample_clips(clips, starts, flips, NUM_FRAMES, 1, **kw), host.sample_clips(clips, starts, flips, NUM_FRAMES, 1, **kw))
    a = dev.sample_clips(clips, starts, flips, NUM_FRAMES, 1, generator=torch.Generator("cuda").manual_seed(3))
    b = host.sample_clips(clips, starts, flips, NUM_FRAMES, 1, generator=torch.Generator("cuda").manual_seed(3))
    assert torch.equal(a, b)
    rows = np.array([29, 0, 7, 7], dtype=np.int64)
    assert torch.equal(dev.moments(rows), host.moments(rows)) and torch.equal(dev.sample_frames(rows, seed=9), host.sample_frames(rows, seed=9))
    with pytest.raises(latte_amd.LatteError):
        dev.moments([30])


# ------------------------------------------------------------------------------------------------ drivers
def _losses(stdout):
    return [line.split("Train Loss: ")[1].split(",")[0] for line in stdout.splitlines() if "Train Loss" in line]


@pytest.mark.gpu
def test_drivers_moments_run_equals_raw_run(enc, tmp_path):
    """tools/encode_clips.py --moments on three small raw clips, then tools/train.py for four steps on `moments_path` and on the raw clips
    with the same seed: finite losses and a checkpoint from both, and -- fp32 store, e == 0 -- the same printed losses."""
    from safetensors.torch import save_file
    from latte_amd.random_init import vae_encoder_state_dict
    vdir = tmp_path / "pretrained" / "vae"
    vdir.mkdir(parents=True)
    save_file({k: v.contiguous() for k, v in vae_encoder_state_dict(0).items()}, str(vdir / "diffusion_pytorch_model.safetensors"))
    raw, mom = tmp_path / "raw", tmp_path / "moments"
    raw.mkdir()
    rng = np.random.default_rng(0)
    for i, (frames, hs, ws) in enumerate([(9, 36, 48), (12, 128, 128), (10, 40, 60)]):
        np.save(raw / f"{i + 1}_clip{i}.npy", rng.integers(0, 256, (frames, hs, ws, 3), dtype=np.uint8))
    cfg_raw = open(os.path.join(ROOT, "configs", "tiny_train_raw.yaml")).read()
    cfg_raw = cfg_raw.replace('data_path: "./raw_clips"', f'data_path: "{raw}"')
    cfg_raw = cfg_raw.replace('pretrained_model_path: "./pretrained"', f'pretrained_model_path: "{tmp_path / "pretrained"}"')
    cfg_mom = open(os.path.join(ROOT, "configs", "tiny_train_moments.yaml")).read()
    cfg_mom = cfg_mom.replace('moments_path: "./moment_clips"', f'moments_path: "{mom}"')
    assert str(raw) in cfg_raw and str(mom) in cfg_mom
    (tmp_path / "raw.yaml").write_text(cfg_raw)
    (tmp_path / "mom.yaml").write_text(cfg_mom)

    def run(*cmd):
        r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, *cmd], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        return r.stdout

    out = run(os.path.join(ROOT, "tools", "encode_clips.py"), "--moments", "--config", str(tmp_path / "mom.yaml"), "--vae", str(vdir),
              "--src", str(raw), "--dst", str(mom), "--dtype", "fp32", "--max-frames", "4")
    assert sorted(os.listdir(mom)) == ["1_clip0.npy", "2_clip1.npy", "3_clip2.npy"], out
    assert np.load(mom / "1_clip0.npy").shape == (9, 2, 8, 16, 16) and np.load(mom / "1_clip0.npy").dtype == np.float32
    losses = {}
    for name in ("mom", "raw"):
        o = run(os.path.join(ROOT, "tools", "train.py"), "--config", str(tmp_path / f"{name}.yaml"), "--out", str(tmp_path / f"run_{name}"),
                "--max-steps", "4", "--log-every", "1")
        losses[name] = _losses(o)
        assert len(losses[name]) == 4 and all(math.isfinite(float(v)) for v in losses[name]), o
        assert os.path.exists(tmp_path / f"run_{name}" / "checkpoints" / "0000004.pt")
        assert ("Moment store: 3 clips, 31 frames x 2 planes, fp32" in o) == (name == "mom")
    print("moments run losses:", losses["mom"], "raw run losses:", losses["raw"], "e =", enc.e)
    if enc.e == 0:
        assert losses["mom"] == losses["raw"]
