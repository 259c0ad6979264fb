"""latte_amd.video_transforms on the host: the temporal window and frame indices, the launch plan (intermediate size, crop
offsets, source region), the dataset -> pipeline mapping and the crop error, against tests/golden/video_transforms.npz -- what the
reference's own datasets/video_transforms.py computed (tools/make_video_transform_golden.py).  No kernel runs here; the plan is the
library's host code, and a numpy restatement of the kernel's arithmetic on that plan is checked against the golden pixels."""
import json
import os
import random
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _util import GOLDEN


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "video_transforms.npz"))


def _cases(gold, name):
    return json.loads(bytes(gold[name]).decode())


def test_temporal_crop_and_frame_indices_match_reference(lib, gold):
    from latte_amd.video_transforms import TemporalRandomCrop, frame_indices
    size, num_frames, seed = (int(v) for v in gold["temporal_params"])
    windows = gold["temporal_windows"]
    totals = set(int(t) for t in windows[:, 0])
    assert min(totals) < size and size + 1 in totals and max(totals) > size + 1      # below, equal to and above size + 1
    crop = TemporalRandomCrop(size, rng=random.Random(seed))
    for (total, begin, end), want in zip(windows.tolist(), gold["temporal_indices"]):
        got = crop(total)
        assert got == (begin, end), (total, got, begin, end)
        idx = frame_indices(*got, num_frames)
        assert idx.dtype.kind == "i" and np.array_equal(idx, want)
    # the reference's off-by-one: with total = size + 1 the window [1, size + 1) is never drawn
    crop = TemporalRandomCrop(size, rng=random.Random(0))
    assert {crop(size + 1) for _ in range(200)} == {(0, size)}
    assert {crop(size + 2)[0] for _ in range(200)} == {0, 1}


def _plan_tuple(p):
    return [p.mid_h, p.mid_w, p.crop_i, p.crop_j, p.reg_y, p.reg_x]


def test_plan_matches_reference_geometry(lib, gold):
    """Intermediate sizes, crop offsets and crop regions.  240 x 320 -> 256 is the round-half-even case: the intermediate is
    256 x 341, (341 - 256) / 2 = 42.5, Python's round gives 42 where round-half-up would give 43."""
    from latte_amd import video_transforms as vt
    cases = _cases(gold, "geometry_cases")
    assert [c for c in cases if c[0] == "ucf"][:3] == [["ucf", 240, 320, 256], ["ucf", 321, 240, 256], ["ucf", 37, 53, 16]]
    for (kind, hs, ws, s), want in zip(cases, gold["geometry"].tolist()):
        p = vt.plan(vt.KIND_UCF_CENTER_CROP if kind == "ucf" else vt.KIND_CENTER_CROP_RESIZE, hs, ws, s, s)
        assert _plan_tuple(p) == want, (kind, hs, ws, s, _plan_tuple(p), want)
        assert (p.out_h, p.out_w) == (s, s)
    p = vt.plan(vt.KIND_UCF_CENTER_CROP, 240, 320, 256, 256)
    assert (p.mid_h, p.mid_w, p.crop_i, p.crop_j) == (256, 341, 0, 42)
    assert p.scale_w == np.float32(1.0 / (256 / 240))          # the GIVEN scale's reciprocal, not 320 / 341
    p = vt.plan(vt.KIND_CENTER_CROP_RESIZE, 180, 320, 128, 128)
    assert (p.reg_y, p.reg_x, p.reg_h, p.reg_w) == (0, 70, 180, 180) and p.scale_h == np.float32(180) / np.float32(128)
    p = vt.plan(vt.KIND_NONE, 24, 18)
    assert (p.out_h, p.out_w, p.scale_h, p.scale_w) == (24, 18, 1.0, 1.0)
    with pytest.raises(vt.LatteError):
        vt.plan(vt.KIND_NONE, 24, 18, 16, 16)
    with pytest.raises(vt.LatteError):
        vt.plan(7, 24, 18, 16, 16)


def test_intermediate_smaller_than_crop_raises_like_reference(lib, gold):
    """short * (256 / short) in double falls below 256 for some short edges (49 is the first); torch floors it to 255 and the
    reference's center_crop raises.  The same short edges raise here, with the same message, and no other below 400."""
    from latte_amd import video_transforms as vt
    raising = [int(v) for v in gold["ucf256_raising_short_edges"]]
    assert raising and raising[0] == 49 and 240 not in raising
    got = []
    for short in range(1, 400):
        try:
            vt.plan(vt.KIND_UCF_CENTER_CROP, short, short + 3, 256, 256)
        except ValueError as e:
            assert str(e) == "height and width must be no smaller than crop_size"
            got.append(short)
    assert got == raising
    # torch itself, on this host: the intermediate of a 49 x 52 clip is 255 rows
    y = F.interpolate(torch.zeros(1, 1, 49, 52), scale_factor=256 / 49, mode="bilinear", align_corners=False)
    assert y.shape[-2] == 255
    with pytest.raises(ValueError, match="height and width must be no smaller than crop_size"):
        vt.plan(vt.KIND_UCF_CENTER_CROP, 52, 49, 256, 256)


def test_get_transform_maps_datasets_like_reference(lib):
    from latte_amd import video_transforms as vt

    def args(name):
        return SimpleNamespace(dataset=name, num_frames=16, frame_interval=3, image_size=256)

    for name in ("ffs", "ffs_img", "ucf101", "ucf101_img"):
        t, ts = vt.get_transform(args(name))
        assert t.kind == vt.KIND_UCF_CENTER_CROP and type(t.spatial) is vt.UCFCenterCropVideo and t.spatial.size == (256, 256)
        assert isinstance(t.flip, vt.RandomHorizontalFlipVideo) and t.flip.p == 0.5
        assert isinstance(ts, vt.TemporalRandomCrop) and ts.size == 48
    for name in ("taichi", "taichi_img"):
        t, _ = vt.get_transform(args(name))
        assert t.kind == vt.KIND_NONE and t.spatial is None and isinstance(t.flip, vt.RandomHorizontalFlipVideo)
    for name in ("sky", "sky_img"):
        t, _ = vt.get_transform(args(name))
        assert t.kind == vt.KIND_CENTER_CROP_RESIZE and type(t.spatial) is vt.CenterCropResizeVideo and t.flip is None   # no flip for sky
    for name in ("synthetic", "kinetics", ""):
        with pytest.raises(NotImplementedError):
            vt.get_transform(args(name))
    # the window and the coin come from the caller's generator
    t, ts = vt.get_transform(args("ucf101"), rng=random.Random(5))
    r = random.Random(5)
    assert ts(200) == (lambda b: (b, b + 48))(r.randint(0, 200 - 48 - 1))
    assert t.draw_flips(3) == [r.random() < 0.5 for _ in range(3)]


def test_transform_refuses_cpu_tensors(lib):
    from latte_amd import video_transforms as vt
    t = vt.VideoTransform(vt.UCFCenterCropVideo(16))
    with pytest.raises(vt.LatteError):
        t(torch.zeros(2, 20, 24, 3, dtype=torch.uint8))


def restate(x, p, flip):
    """The kernel's arithmetic (latte_amd/csrc/video.hip) in numpy fp32 on the plan p: x uint8 [N, Hs, Ws, 3] -> [N, 3, out_h, out_w]."""
    f32 = np.float32

    def taps(scale, crop, n_out, size):
        d = np.arange(n_out, dtype=np.int64) + crop
        r = f32(scale) * (d.astype(f32) + f32(0.5)) - f32(0.5)
        r = np.maximum(r, f32(0))
        a = np.minimum(r.astype(np.int64), size - 1)
        lam = np.clip(r - a.astype(f32), f32(0), f32(1)).astype(f32)
        return a, a + (a < size - 1), lam

    ya, yb, ly = taps(p.scale_h, p.crop_i, p.out_h, p.reg_h)
    xa, xb, lx = taps(p.scale_w, p.crop_j, p.out_w, p.reg_w)
    ca, cb = p.reg_x + xa, p.reg_x + xb
    if flip:                                                    # the frame is mirrored BEFORE the crop and the resize
        ca, cb = p.src_w - 1 - ca, p.src_w - 1 - cb
    s = (x.astype(f32) / f32(255)).transpose(0, 3, 1, 2)
    ra, rb = s[:, :, p.reg_y + ya], s[:, :, p.reg_y + yb]
    wx0, wy0 = f32(1) - lx, (f32(1) - ly)[:, None]
    top = ra[..., ca] * wx0 + ra[..., cb] * lx
    bot = rb[..., ca] * wx0 + rb[..., cb] * lx
    return ((top * wy0 + bot * ly[:, None]) - f32(0.5)) / f32(0.5)


_KINDS = {"ucf101": 1, "ffs": 1, "sky": 2, "taichi": 0}


def test_plan_and_arithmetic_reproduce_reference_pixels(lib, gold):
    """The golden pixels of the reference's three Compose pipelines from the plan plus the kernel's arithmetic restated in numpy:
    flipped and not.  The flip mirrors the SOURCE columns.  Mirroring the output instead is not the same thing in general: in the
    37 x 48 -> 16 case the scale_factor resize anchors its 20 intermediate columns at the left edge (they reach source column
    44.6 of 47), so the flipped clip shows other pixels -- asserted below; for taichi (no resize) the two agree."""
    from latte_amd import video_transforms as vt
    worst = 0.0
    for k, (dataset, n, hs, ws, s) in enumerate(_cases(gold, "pixel_cases")):
        x = gold[f"pixel{k}_in"]
        assert x.shape == (n, hs, ws, 3) and x.dtype == np.uint8
        p = vt.plan(_KINDS[dataset], hs, ws, s, s)
        flips = [False] + ([True] if dataset != "sky" else [])
        for fl in flips:
            want = gold[f"pixel{k}_out_flipped" if fl else f"pixel{k}_out"]
            got = restate(x, p, fl)
            assert got.shape == want.shape and got.dtype == np.float32
            worst = max(worst, float(np.abs(got - want).max()))
    print("numpy restatement vs reference pipelines, max abs:", worst)
    assert worst <= 1e-6
    assert np.abs(gold["pixel0_out_flipped"] - gold["pixel0_out"][..., ::-1]).max() > 1e-2       # ucf101 37 x 48 -> 16
    taichi = [k for k, c in enumerate(_cases(gold, "pixel_cases")) if c[0] == "taichi"][0]
    assert np.array_equal(gold[f"pixel{taichi}_out_flipped"], gold[f"pixel{taichi}_out"][..., ::-1])
