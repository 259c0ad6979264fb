"""The reference's ``datasets/video_transforms.py`` for the call sites of ``datasets/__init__.py:13-76``, on the MI355X:

    temporal_sample = video_transforms.TemporalRandomCrop(args.num_frames * args.frame_interval)
    transform = transforms.Compose([ToTensorVideo(), RandomHorizontalFlipVideo(), UCFCenterCropVideo(args.image_size),
                                    transforms.Normalize(mean=[0.5, 0.5, 0.5], std=[0.5, 0.5, 0.5], inplace=True)])

becomes ``transform, temporal_sample = get_transform(args)``, and ``transform(frames_uint8_cuda)`` is ONE launch of
``latte_video_transform`` (latte_amd/csrc/video.hip): gathered uint8 frames [N, Hs, Ws, 3] -> fp32 [N, 3, S, S] in [-1, 1], what
``AutoencoderKL.encode`` consumes.  The crop offsets, the intermediate size and the coordinate scales are worked out on the host by
``latte_video_transform_plan`` (``plan`` below), the same code the launch uses.  Video DECODING (decord / torchvision.io) is not
offered: frames arrive as uint8 arrays.  There is no CPU fallback.
"""
import random

import numpy as np
import torch

from . import _lib
from ._lib import LatteError, check, load_library, ptr, stream_ptr

KIND_NONE, KIND_UCF_CENTER_CROP, KIND_CENTER_CROP_RESIZE = 0, 1, 2
_CROP_ERROR = "height and width must be no smaller than crop_size"


class TemporalRandomCrop:
    """``TemporalRandomCrop(size)(total_frames) -> (begin, end)`` with the reference's off-by-one (the last possible window start
    is never drawn: ``rand_end = max(0, total - size - 1)``).  Draws from ``rng`` (a ``random.Random``; default: the ``random``
    module, as the reference)."""

    def __init__(self, size, rng=None):
        self.size = size
        self.rng = rng if rng is not None else random

    def __call__(self, total_frames):
        rand_end = max(0, total_frames - self.size - 1)
        begin_index = self.rng.randint(0, rand_end)
        end_index = min(begin_index + self.size, total_frames)
        return begin_index, end_index


def frame_indices(start, end, num_frames):
    """The frames a dataset reads of the window [start, end): ``np.linspace(start, end - 1, num_frames, dtype=int)``."""
    return np.linspace(start, end - 1, num_frames, dtype=int)


def _size(size):
    if isinstance(size, tuple):
        if len(size) != 2:
            raise ValueError(f"size should be tuple (height, width), instead got {size}")
        return size
    return (size, size)


class UCFCenterCropVideo:
    """Scale the short edge to ``size`` (bilinear, torch's scale_factor form), then center crop."""
    kind = KIND_UCF_CENTER_CROP

    def __init__(self, size, interpolation_mode="bilinear"):
        if interpolation_mode != "bilinear":
            raise LatteError("latte_amd.video_transforms resizes with bilinear interpolation only")
        self.size = _size(size)
        self.interpolation_mode = interpolation_mode

    def __repr__(self):
        return f"{self.__class__.__name__}(size={self.size}, interpolation_mode={self.interpolation_mode}"


class CenterCropResizeVideo(UCFCenterCropVideo):
    """Center crop to the short edge, then resize to ``size`` (bilinear)."""
    kind = KIND_CENTER_CROP_RESIZE


class RandomHorizontalFlipVideo:
    """The flip coin of one clip: ``draw()`` is ``random.random() < p`` on ``rng`` (default: the ``random`` module)."""

    def __init__(self, p=0.5, rng=None):
        self.p = p
        self.rng = rng if rng is not None else random

    def draw(self):
        return self.rng.random() < self.p

    def __repr__(self):
        return f"{self.__class__.__name__}(p={self.p})"


def plan(kind, src_h, src_w, out_h=0, out_w=0):
    """The host side of one launch (``latte_video_plan`` of include/latte_amd.h): intermediate size, crop offsets, source region
    and coordinate scales.  Raises the reference's ValueError when the scaled clip is smaller than the crop."""
    p = _lib.VideoPlan()
    lib = load_library()
    rc = lib.latte_video_transform_plan(int(kind), int(src_h), int(src_w), int(out_h), int(out_w), p)
    if rc != 0 and (lib.latte_last_error() or b"").decode() == _CROP_ERROR:
        raise ValueError(_CROP_ERROR)
    check(rc)
    return p


class VideoTransform:
    """``Compose([ToTensorVideo(), flip, spatial, Normalize(0.5, 0.5)])`` as one launch.  ``spatial``: ``UCFCenterCropVideo``,
    ``CenterCropResizeVideo`` or None (keep the size); ``flip``: a ``RandomHorizontalFlipVideo`` or None (the sky pipeline has none).

    ``transform(frames, flip=None)``: frames uint8 on the GPU, [B, F, Hs, Ws, 3] (B clips) or [N, Hs, Ws, 3] (one clip) ->
    fp32 [B, F, 3, S_h, S_w] / [N, 3, S_h, S_w].  ``flip``: a bool or one bool per clip; None draws one coin per clip from the
    composed ``RandomHorizontalFlipVideo`` (all frames of a clip share it, as in the reference)."""

    def __init__(self, spatial=None, flip=None):
        if spatial is not None and not isinstance(spatial, UCFCenterCropVideo):
            raise LatteError("spatial must be UCFCenterCropVideo, CenterCropResizeVideo or None")
        self.spatial, self.flip = spatial, flip
        self.kind = KIND_NONE if spatial is None else spatial.kind

    def output_size(self, src_h, src_w):
        return (src_h, src_w) if self.spatial is None else tuple(self.spatial.size)

    def draw_flips(self, clips):
        return [self.flip.draw() if self.flip is not None else False for _ in range(clips)]

    def __call__(self, frames, flip=None):
        _lib.require_gpu()
        if not torch.is_tensor(frames) or frames.dtype != torch.uint8 or frames.dim() not in (4, 5) or frames.shape[-1] != 3:
            raise LatteError("frames must be a uint8 tensor [B, F, Hs, Ws, 3] or [N, Hs, Ws, 3]")
        if frames.device.type != "cuda":
            raise LatteError("latte_amd.video_transforms runs on an MI355X only: pass frames on 'cuda' (there is no CPU fallback)")
        batched = frames.dim() == 5
        clips, per_clip = (frames.shape[0], frames.shape[1]) if batched else (1, frames.shape[0])
        hs, ws = frames.shape[-3], frames.shape[-2]
        if clips * per_clip == 0:
            raise LatteError("frames must hold at least one frame")
        out_h, out_w = self.output_size(hs, ws)
        plan(self.kind, hs, ws, out_h, out_w)             # the reference's ValueError, before anything is allocated
        if flip is None:
            flip = self.draw_flips(clips)
        elif isinstance(flip, (bool, int)):
            flip = [bool(flip)] * clips
        flip = [bool(v) for v in (flip.tolist() if torch.is_tensor(flip) else flip)]
        if len(flip) != clips:
            raise LatteError(f"flip must be one bool per clip ({clips}), got {len(flip)}")
        src = frames.contiguous()
        n = clips * per_clip
        out = torch.empty(n, 3, out_h, out_w, device=frames.device, dtype=torch.float32)
        fl = None
        if any(flip):
            fl = torch.tensor(flip, dtype=torch.uint8).repeat_interleave(per_clip).to(frames.device)
        with torch.cuda.device(frames.device):
            check(load_library().latte_video_transform(ptr(src), n, hs, ws, self.kind, out_h, out_w, ptr(fl), ptr(out), stream_ptr()))
        return out.view(clips, per_clip, 3, out_h, out_w) if batched else out

    def __repr__(self):
        return f"VideoTransform(spatial={self.spatial!r}, flip={self.flip!r})"


_UCF = ("ffs", "ffs_img", "ucf101", "ucf101_img")
_TAICHI = ("taichi", "taichi_img")
_SKY = ("sky", "sky_img")


def get_transform(args, rng=None):
    """``(transform, temporal_sample)`` of ``datasets.get_dataset(args)`` (datasets/__init__.py:13-76) for ``args.dataset``; the
    ``_img`` variants get their video part.  ``rng``: the ``random.Random`` the temporal window and the flip coin draw from."""
    temporal_sample = TemporalRandomCrop(args.num_frames * args.frame_interval, rng=rng)
    if args.dataset in _UCF:
        return VideoTransform(UCFCenterCropVideo(args.image_size), RandomHorizontalFlipVideo(rng=rng)), temporal_sample
    if args.dataset in _TAICHI:
        return VideoTransform(None, RandomHorizontalFlipVideo(rng=rng)), temporal_sample
    if args.dataset in _SKY:
        return VideoTransform(CenterCropResizeVideo(args.image_size), None), temporal_sample
    raise NotImplementedError(args.dataset)
