"""latte_video_transform on the GPU (latte_amd/csrc/video.hip) against torch itself on the CPU -- F.interpolate on x.float() / 255, the
crop, the flip, the normalise -- and against the committed output of the reference's own classes (tests/golden/video_transforms.npz)
at the small shapes; then AutoencoderKL.encode_video_raw and the training driver on raw clips.

Bound: max abs difference <= 1e-5 on the [-1, 1] output.  With identical source coordinates what remains is fp32 re-association of the
blend, about 1e-6; one coordinate that slips by an ulp moves a blend weight by up to 3e-5 and the output by about 1e-4: 1e-5 separates
the two."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _util import GOLDEN, rel_l2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 1e-5
UCF, SKY, NONE = "ucf", "sky", "none"


def torch_pipeline(frames, kind, size, flips):
    """frames uint8 [N, Hs, Ws, 3] (CPU), flips one bool per frame -> fp32 [N, 3, S, S]: ToTensorVideo, hflip, the spatial transform
    and Normalize(0.5, 0.5) in torch, as datasets/video_transforms.py composes them."""
    x = frames.permute(0, 3, 1, 2).float() / 255.0
    x = torch.stack([f.flip(-1) if fl else f for f, fl in zip(x, flips)])
    h, w = x.shape[-2:]
    if kind == UCF:
        x = F.interpolate(x, scale_factor=size / min(h, w), mode="bilinear", align_corners=False)
        h, w = x.shape[-2:]
        assert h >= size and w >= size
        i, j = int(round((h - size) / 2.0)), int(round((w - size) / 2.0))
        x = x[..., i:i + size, j:j + size]
    elif kind == SKY:
        if h < w:
            j = int(round((w - h) / 2.0))
            x = x[..., :, j:j + h]
        else:
            i = int(round((h - w) / 2.0))
            x = x[..., i:i + w, :]
        x = F.interpolate(x, size=(size, size), mode="bilinear", align_corners=False)
    return x.contiguous().sub_(0.5).div_(0.5)


def make_transform(kind, size):
    from latte_amd import video_transforms as vt
    spatial = {UCF: vt.UCFCenterCropVideo, SKY: vt.CenterCropResizeVideo}.get(kind)
    return vt.VideoTransform(spatial(size) if spatial else None)


def frames_u8(shape, seed):
    return torch.randint(0, 256, (*shape, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


CASES = {
    # name: (kind, frames, Hs, Ws, size)
    "ucf_landscape_upscale": (UCF, 4, 240, 320, 256),
    "ucf_portrait_downscale": (UCF, 2, 300, 200, 128),
    "sky_landscape": (SKY, 3, 180, 320, 128),
    "sky_portrait_odd": (SKY, 2, 45, 28, 24),
    "taichi": (NONE, 2, 64, 64, 64),
    "border_every_clamp": (UCF, 1, 5, 7, 8),
    "taichi_width_50_scalar_stores": (NONE, 2, 30, 50, 0),       # out_w % 4 == 2: the scalar-store tail
    "ucf_out_18_scalar_stores": (UCF, 2, 40, 27, 18),            # out_w % 4 == 2 with a resize
    "sky_out_13_odd_everything": (SKY, 1, 31, 36, 13),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_transform_vs_torch(lib, name):
    kind, n, hs, ws, size = CASES[name]
    x = frames_u8((n, hs, ws), seed=len(name) + hs)
    for flip in (False, True):
        want = torch_pipeline(x, kind, size, [flip] * n)
        got = make_transform(kind, size)(x.cuda(), flip=flip).cpu()
        assert got.shape == want.shape and got.dtype == torch.float32
        err = float((got - want).abs().max())
        print(f"{name} flip={flip}: max abs {err:.3e}")
        assert err <= BOUND, (name, flip, err)
        assert float(got.abs().max()) <= 1.0


@pytest.mark.gpu
def test_exact_2x_downscale_matches_to_blend_rounding(lib):
    """512 -> 256: every source coordinate is k + 0.5 exactly, every weight 0.5, every product exact, so the only roundings are the
    division x / 255 and the three sums of the blend, each at most half an ulp of a value below 1 (6e-8) and doubled by the
    normalise: 2.4e-7 covers two of them on each side."""
    x = frames_u8((1, 512, 512), seed=2)
    want = torch_pipeline(x, UCF, 256, [False])
    got = make_transform(UCF, 256)(x.cuda()).cpu()
    err = float((got - want).abs().max())
    print(f"exact 2x downscale: max abs {err:.3e}")
    assert err <= 2.4e-7, err
    # the same pixels in closed form: the mean of each 2 x 2 block
    blocks = (x.permute(0, 3, 1, 2).double() / 255).reshape(1, 3, 256, 2, 256, 2).mean(dim=(3, 5))
    assert float((got.double() - (blocks - 0.5) / 0.5).abs().max()) <= 2.4e-7


@pytest.mark.gpu
@pytest.mark.parametrize("kind,size", [(UCF, 16), (SKY, 16), (NONE, 0)])
def test_flip_per_clip_in_a_batch(lib, kind, size):
    """[2, 3, Hs, Ws, 3]: the coin is per CLIP -- on, off and mixed -- and mirrors the source frame before the crop and the resize.
    37 x 53 -> 16 has an asymmetric window (the scale_factor resize anchors at the left edge), so mirroring the output instead would
    miss the bound by orders of magnitude."""
    x = frames_u8((2, 3, 37, 53), seed=7)
    t = make_transform(kind, size)
    for flips in ([False, False], [True, True], [True, False], [False, True]):
        want = torch_pipeline(x.reshape(6, 37, 53, 3), kind, size, [f for f in flips for _ in range(3)])
        got = t(x.cuda(), flip=flips).cpu()
        assert got.shape[:3] == (2, 3, 3)
        err = float((got.reshape(want.shape) - want).abs().max())
        print(f"{kind} flips={flips}: max abs {err:.3e}")
        assert err <= BOUND, (kind, flips, err)
    assert torch.equal(t(x.cuda(), flip=torch.tensor([True, False])), t(x.cuda(), flip=[True, False]))
    assert torch.equal(t(x.cuda(), flip=None), t(x.cuda(), flip=False))          # no RandomHorizontalFlipVideo composed: no coin
    from latte_amd.video_transforms import LatteError
    with pytest.raises(LatteError):
        t(x.cuda(), flip=[True])


@pytest.mark.gpu
def test_composed_coin_is_drawn_per_clip(lib):
    import random
    from types import SimpleNamespace
    from latte_amd import video_transforms as vt
    args = SimpleNamespace(dataset="ucf101", num_frames=3, frame_interval=1, image_size=16)
    t, _ = vt.get_transform(args, rng=random.Random(12))
    r = random.Random(12)
    coins = [r.random() < 0.5 for _ in range(4)]
    assert True in coins and False in coins
    x = frames_u8((4, 3, 20, 31), seed=8).cuda()
    assert torch.equal(t(x), make_transform(UCF, 16)(x, flip=coins))


@pytest.mark.gpu
def test_transform_vs_reference_golden(lib):
    """The committed outputs of the reference's own Compose pipelines (tools/make_video_transform_golden.py), flipped and not."""
    z = np.load(os.path.join(GOLDEN, "video_transforms.npz"))
    kinds = {"ucf101": UCF, "ffs": UCF, "sky": SKY, "taichi": NONE}
    for k, (dataset, n, hs, ws, s) in enumerate(json.loads(bytes(z["pixel_cases"]).decode())):
        x = torch.from_numpy(z[f"pixel{k}_in"]).cuda()
        t = make_transform(kinds[dataset], s)
        for fl in [False] + ([True] if dataset != "sky" else []):
            want = torch.from_numpy(z[f"pixel{k}_out_flipped" if fl else f"pixel{k}_out"])
            got = t(x, flip=fl).cpu()
            err = float((got - want).abs().max())
            print(f"golden {dataset} {hs}x{ws}->{s} flip={fl}: max abs {err:.3e}")
            assert got.shape == want.shape and err <= BOUND, (dataset, fl, err)


@pytest.mark.gpu
def test_crop_error_and_bad_input(lib):
    from latte_amd import video_transforms as vt
    t = make_transform(UCF, 256)
    with pytest.raises(ValueError, match="height and width must be no smaller than crop_size"):
        t(torch.zeros(1, 49, 60, 3, dtype=torch.uint8, device="cuda"))
    with pytest.raises(vt.LatteError):
        t(torch.zeros(1, 49, 60, 3, device="cuda"))
    with pytest.raises(vt.LatteError):
        t(torch.zeros(1, 3, 49, 60, dtype=torch.uint8, device="cuda"))


# ------------------------------------------------------------------------------------------------ encoder
def _encoder(frames, seed):
    from latte_amd.random_init import vae_encoder_state_dict
    from latte_amd.vae import AutoencoderKL
    vae = AutoencoderKL(max_frames=frames, with_encoder=True)
    vae.load_state_dict(vae_encoder_state_dict(seed))
    return vae.to("cuda")


@pytest.mark.gpu
def test_encode_video_raw_bits_and_uint8_path(lib):
    vae = _encoder(6, seed=4)
    t = make_transform(UCF, 128)
    x = frames_u8((2, 3, 150, 200), seed=9).cuda()
    # the same kernels on the same input: bit for bit
    pre = t(x, flip=[True, False]).reshape(6, 3, 128, 128)
    want = vae.encode(pre).latent_dist.sample(generator=torch.Generator("cuda").manual_seed(5)).mul_(vae.config.scaling_factor)
    got = vae.encode_video_raw(x, t, flip=[True, False], generator=torch.Generator("cuda").manual_seed(5))
    assert got.shape == (2, 3, 4, 16, 16) and torch.isfinite(got).all()
    assert torch.equal(got.reshape(6, 4, 16, 16), want)
    # Hs == Ws == S, no flip: the transform is x / 255 -> (v - 0.5) / 0.5 where encode_video_uint8 reads x / 127.5 - 1
    sq = frames_u8((2, 3, 128, 128), seed=10).cuda()
    a = vae.encode_video_raw(sq, t, flip=False, generator=torch.Generator("cuda").manual_seed(6))
    b = vae.encode_video_uint8(sq, generator=torch.Generator("cuda").manual_seed(6))
    err = rel_l2(a, b)
    print(f"encode_video_raw vs encode_video_uint8 at Hs == Ws == S: rel L2 {err:.3e}")
    assert a.shape == b.shape and err < 1e-3


# ------------------------------------------------------------------------------------------------ driver
@pytest.mark.gpu
def test_train_driver_on_raw_clips(tmp_path):
    """tools/train.py on configs/tiny_train_raw.yaml: raw clips of mixed lengths and sizes, 3 steps, finite losses, and the same
    losses again from the same seed (window, coin and posterior noise all come from seeded generators)."""
    from safetensors.torch import save_file
    from latte_amd.random_init import vae_encoder_state_dict
    vdir = tmp_path / "pretrained" / "vae"
    vdir.mkdir(parents=True)
    save_file({k: v.contiguous() for k, v in vae_encoder_state_dict(0).items()}, str(vdir / "diffusion_pytorch_model.safetensors"))
    data = tmp_path / "clips"
    data.mkdir()
    rng = np.random.default_rng(0)
    for i, (frames, hs, ws) in enumerate([(4, 128, 128), (9, 150, 200), (23, 260, 131), (12, 144, 176)]):
        np.save(data / f"{i % 5}_clip{i}.npy", rng.integers(0, 256, (frames, hs, ws, 3), dtype=np.uint8))
    cfg = open(os.path.join(ROOT, "configs", "tiny_train_raw.yaml")).read()
    cfg = cfg.replace('data_path: "./raw_clips"', f'data_path: "{data}"')
    cfg = cfg.replace('pretrained_model_path: "./pretrained"', f'pretrained_model_path: "{tmp_path / "pretrained"}"')
    assert str(data) in cfg and str(tmp_path / "pretrained") in cfg
    (tmp_path / "cfg.yaml").write_text(cfg)
    runs = []
    for k in range(2):
        r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "tools", "train.py"), "--config",
                            str(tmp_path / "cfg.yaml"), "--out", str(tmp_path / f"run{k}"), "--max-steps", "3", "--log-every", "1"],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        losses = [float(line.split("Train Loss: ")[1].split(",")[0]) for line in r.stdout.splitlines() if "Train Loss" in line]
        assert len(losses) == 3 and all(math.isfinite(v) for v in losses), r.stdout
        runs.append(losses)
    print("raw-clip driver losses:", runs[0])
    assert runs[0] == runs[1]
