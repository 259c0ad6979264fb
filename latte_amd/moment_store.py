"""Training from STORED VAE moments: every frame of every clip is encoded once, under each flip, and its
posterior moments ``[mean | logvar]`` are kept; a training batch is then a gather of rows plus ``(mean + std * noise) * 0.18215`` in one
launch of ``latte_moment_sample`` (latte_amd/csrc/moments.hip) -- the reference's per-step ``TemporalRandomCrop`` window, flip coin and
``vae.encode(x).latent_dist.sample().mul_(0.18215)`` (train.py:204-211) with no encoder in the step:

    store = MomentStore.build(vae, clips, transform)            # once; store.save(dir) / MomentStore.load(dir)
    x = store.sample_clips(clip_ids, starts, flips, num_frames, frame_interval, generator=gen)      # every step

Exact only for transforms whose ONLY spatial randomness is the flip (every dataset pipeline of ``video_transforms.get_transform``: the
spatial part is a deterministic centre crop / resize): the transform and the SD-VAE encoder act per frame, so the moments of frame j
under flip f do not depend on the window j is drawn in.  Index arithmetic, ``save`` and ``load`` need no GPU; sampling does, and there
is no CPU fallback.
"""
import ctypes
import glob
import os

import numpy as np
import torch

from . import _lib
from ._lib import LatteError, check, load_library, ptr, stream_ptr
from .train_util import clip_label
from .vae import randn_tensor
from .video_transforms import frame_indices

SEED_NONE = 2 ** 64 - 1          # LATTE_SEED_NONE of include/latte_amd.h
_DTYPES = {"f16": torch.float16, "fp16": torch.float16, "float16": torch.float16, "fp32": torch.float32, "float32": torch.float32}


class MomentStore:
    """Rows ``[n_rows, 8, h * w]`` (f16 or fp32), row ``(first_frame[clip] + frame) * P + plane``: P = 1 (plane 0, unflipped) or
    2 (plane 1 = horizontally flipped), on the GPU (``device="cuda"``, the resident store) or in host memory (``device="cpu"``: the
    requested rows are gathered into a pinned buffer and uploaded per call, then the same kernel runs on them)."""

    def __init__(self, clips, names, device="cpu"):
        """clips: per clip a tensor / array [T, P, 8, h, w], all of one dtype, P, h and w; names: their file stems."""
        clips = [torch.as_tensor(np.asarray(c)) if not torch.is_tensor(c) else c for c in clips]
        if not clips or len(clips) != len(names):
            raise LatteError("MomentStore: needs at least one clip and one name per clip")
        first = clips[0]
        for c, n in zip(clips, names):
            if c.dim() != 5 or c.shape[2] != 8 or c.shape[0] < 1 or c.shape[1] not in (1, 2):
                raise LatteError(f"MomentStore: {n}: a clip's moments are [T, P (1 | 2), 8, h, w], got {tuple(c.shape)}")
            if c.shape[1:] != first.shape[1:] or c.dtype != first.dtype:
                raise LatteError(f"MomentStore: {n}: {c.dtype} {tuple(c.shape[1:])} differs from the first clip's {first.dtype} {tuple(first.shape[1:])}")
        if first.dtype not in (torch.float16, torch.float32):
            raise LatteError(f"MomentStore: moments are f16 or fp32, got {first.dtype}")
        self.names = [str(n) for n in names]
        self.latent_hw = (int(first.shape[3]), int(first.shape[4]))
        self._planes = int(first.shape[1])
        self._frames = np.array([c.shape[0] for c in clips], dtype=np.int64)
        self._first = np.concatenate([[0], np.cumsum(self._frames)[:-1]]).astype(np.int64)
        hw = self.latent_hw[0] * self.latent_hw[1]
        self._data = torch.cat([c.reshape(-1, 8, hw) for c in clips]).contiguous()
        self._device = torch.device("cpu")
        self.to(device)

    # ------------------------------------------------------------------ construction
    @classmethod
    def build(cls, vae, clips, transform, dtype="f16", planes=None):
        """Encode ``clips`` -- an iterable of (name, uint8 [T, Hs, Ws, 3]) -- once: per clip and plane ``transform(frames, flip=[plane])``
        and the encoder's moments (``AutoencoderKL.encode_video_raw_moments``), ``vae.max_frames`` frames per call.  planes: (False, True)
        when the transform has a flip, (False,) when it has none.  f16 storage is the round-to-nearest half of the fp32 moments.
        The store is returned in host memory: ``.to("cuda")`` makes it resident, ``save(dir)`` writes it."""
        if dtype not in _DTYPES:
            raise LatteError(f"MomentStore.build: dtype must be 'f16' or 'fp32', got {dtype!r}")
        if planes is None:
            planes = (False, True) if getattr(transform, "flip", None) is not None else (False,)
        planes = tuple(bool(p) for p in planes)
        if planes not in ((False,), (False, True)):
            raise LatteError("MomentStore.build: planes is (False,) or (False, True)")
        out, names = [], []
        for name, frames in clips:
            frames = torch.as_tensor(np.ascontiguousarray(frames)) if not torch.is_tensor(frames) else frames
            if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[-1] != 3 or frames.shape[0] < 1:
                raise LatteError(f"MomentStore.build: {name}: clips are uint8 [T, Hs, Ws, 3], got {frames.dtype} {tuple(frames.shape)}")
            per_plane = []
            for plane in planes:
                chunks = [vae.encode_video_raw_moments(frames[s:s + vae.max_frames], transform, flip=[plane])[0]
                          for s in range(0, frames.shape[0], vae.max_frames)]
                per_plane.append(torch.cat(chunks))
            m = torch.stack(per_plane, dim=1)                     # [T, P, 8, h, w] fp32
            out.append(m.to(_DTYPES[dtype]).cpu())
            names.append(name)
        return cls(out, names)

    def save(self, directory):
        """One ``<name>.npy`` [T, P, 8, h, w] per clip (the ``<label>_...`` prefix of the name survives)."""
        os.makedirs(directory, exist_ok=True)
        data = self._data.cpu().numpy()
        h, w = self.latent_hw
        for name, first, t in zip(self.names, self._first, self._frames):
            np.save(os.path.join(directory, name + ".npy"), data[first * self._planes:(first + t) * self._planes].reshape(t, self._planes, 8, h, w))

    @classmethod
    def load(cls, directory, device="cuda"):
        """Map every ``*.npy`` under ``directory`` (sorted by name, as the trainer's data classes list their files) and concatenate."""
        files = sorted(glob.glob(os.path.join(directory, "*.npy")))
        if not files:
            raise LatteError(f"MomentStore.load: no .npy moment files under {directory}")
        arrays = [np.load(f, mmap_mode="r") for f in files]
        for f, a in zip(files, arrays):
            if a.dtype not in (np.float16, np.float32):
                raise LatteError(f"MomentStore.load: {f}: moment files are f16 or fp32 [T, P, 8, h, w], got {a.dtype} {a.shape}")
        return cls([torch.from_numpy(np.array(a)) for a in arrays], [os.path.splitext(os.path.basename(f))[0] for f in files], device)

    def to(self, device):
        device = torch.device(device)
        if device.type == "cuda":
            _lib.require_gpu()
            if device.index is None:
                device = torch.device("cuda", torch.cuda.current_device())
        elif device.type != "cpu":
            raise LatteError("MomentStore lives on 'cuda' or 'cpu'")
        self._data = self._data.to(device)
        self._device = device
        return self

    # ------------------------------------------------------------------ properties
    @property
    def device(self):
        return self._device

    @property
    def num_clips(self):
        return len(self.names)

    @property
    def clip_frames(self):
        return self._frames.tolist()

    @property
    def labels(self):
        return [clip_label(n) for n in self.names]

    @property
    def planes(self):
        return (False, True)[:self._planes]

    @property
    def dtype(self):
        return "f16" if self._data.dtype == torch.float16 else "fp32"

    @property
    def num_rows(self):
        return int(self._data.shape[0])

    @property
    def nbytes(self):
        return self._data.numel() * self._data.element_size()

    # ------------------------------------------------------------------ index arithmetic (host only)
    def frame_rows(self, clip, frames, flip=False):
        """Rows of the given frames of ``clip`` in the plane of ``flip`` -> int64 [len(frames)]."""
        clip = int(clip)
        if not 0 <= clip < self.num_clips:
            raise LatteError(f"MomentStore: clip {clip} is outside the store's {self.num_clips} clips")
        if flip and self._planes == 1:
            raise LatteError("MomentStore: this store holds one plane (built without a flip): flip=True is not available")
        frames = np.asarray(frames, dtype=np.int64).reshape(-1)
        t = int(self._frames[clip])
        if frames.size == 0 or frames.min() < 0 or frames.max() >= t:
            raise LatteError(f"MomentStore: frames {frames.tolist()} leave clip {clip} ({self.names[clip]}: {t} frames)")
        return (self._first[clip] + frames) * self._planes + int(bool(flip))

    def rows(self, clip, start, flip, num_frames, frame_interval):
        """Rows of the window a dataset reads at ``start``: ``frame_indices(start, start + num_frames * frame_interval, num_frames)``
        of ``clip`` in the plane of ``flip`` -> int64 [num_frames]."""
        start, num_frames, frame_interval = int(start), int(num_frames), int(frame_interval)
        if num_frames < 1 or frame_interval < 1:
            raise LatteError("MomentStore: num_frames and frame_interval must be at least 1")
        if 0 <= int(clip) < self.num_clips and (start < 0 or start + num_frames * frame_interval > int(self._frames[int(clip)])):
            raise LatteError(f"MomentStore: the window [{start}, {start + num_frames * frame_interval}) leaves clip {int(clip)} "
                             f"({int(self._frames[int(clip)])} frames)")
        return self.frame_rows(clip, frame_indices(start, start + num_frames * frame_interval, num_frames), flip)

    # ------------------------------------------------------------------ sampling (GPU)
    def _launch(self, rows, what, noise=None, seed=SEED_NONE, offset=0, scale=1.0):
        rows = np.ascontiguousarray(np.asarray(rows, dtype=np.int64).reshape(-1))
        n = int(rows.size)
        if n and (rows.min() < 0 or rows.max() >= self.num_rows):
            raise LatteError(f"MomentStore: rows must lie in [0, {self.num_rows})")
        _lib.require_gpu()
        h, w = self.latent_hw
        if self._device.type == "cuda":
            dev, store, n_rows = self._device, self._data, self.num_rows
        else:                                                   # host-resident: gather into a pinned buffer, upload, rows 0 .. n-1
            dev = torch.device("cuda", torch.cuda.current_device())
            staged = torch.empty((n, 8, h * w), dtype=self._data.dtype, pin_memory=True)
            torch.index_select(self._data, 0, torch.from_numpy(rows), out=staged)
            store, n_rows, rows = staged.to(dev, non_blocking=True), n, np.arange(n, dtype=np.int64)
        if noise is not None:
            if noise.device != dev or noise.dtype != torch.float32 or not noise.is_contiguous() or noise.numel() != n * 4 * h * w:
                raise LatteError(f"MomentStore: noise must be a contiguous fp32 tensor of {(n, 4, h, w)} on {dev}")
        out = torch.empty(n, 8 if what == 0 else 4, h, w, device=dev, dtype=torch.float32)
        with torch.cuda.device(dev):
            check(load_library().latte_moment_sample(ptr(store), int(store.dtype == torch.float16), n_rows, h * w, ctypes.c_void_p(rows.ctypes.data),
                                                     n, ptr(noise), int(seed), int(offset), float(scale), what, ptr(out), stream_ptr()))
        return out

    def moments(self, rows):
        """The gathered moments of ``rows`` -> fp32 [n, 8, h, w] (mean | logvar)."""
        return self._launch(rows, 0)

    def sample_frames(self, rows, generator=None, noise=None, seed=None, scale=None, offset=0):
        """``(mean + std * z) * scale`` of arbitrary rows -> fp32 [n, 4, h, w].  Exactly one noise source: ``generator`` draws
        ``randn_tensor((n, 4, h, w))`` as the encoder's sampling calls do; ``noise`` is the caller's tensor; ``seed`` (with ``offset``)
        draws inside the kernel from the engine's Philox stream.  scale: 0.18215 by default."""
        if sum(v is not None for v in (generator, noise, seed)) != 1:
            raise LatteError("MomentStore: give exactly one of generator, noise and seed")
        rows = np.asarray(rows, dtype=np.int64).reshape(-1)
        scale = 0.18215 if scale is None else scale
        if seed is not None:
            if not 0 <= int(seed) < SEED_NONE:
                raise LatteError("MomentStore: seed must lie in [0, 2^64 - 1)")
            return self._launch(rows, 2, None, seed, offset, scale)
        if generator is not None:
            _lib.require_gpu()
            dev = self._device if self._device.type == "cuda" else torch.device("cuda", torch.cuda.current_device())
            noise = randn_tensor((rows.size, 4, *self.latent_hw), generator=generator, device=dev)
        return self._launch(rows, 2, noise, 0, 0, scale)

    def sample_clips(self, clips, starts, flips, num_frames, frame_interval, generator=None, noise=None, seed=None, scale=None):
        """One window per entry of ``clips`` / ``starts`` / ``flips`` -> latents fp32 [n, num_frames, 4, h, w], one launch."""
        clips, starts, flips = list(clips), list(starts), list(flips)
        if not clips or len(starts) != len(clips) or len(flips) != len(clips):
            raise LatteError("MomentStore: clips, starts and flips need one entry per clip, at least one")
        rows = np.concatenate([self.rows(c, s, f, num_frames, frame_interval) for c, s, f in zip(clips, starts, flips)])
        out = self.sample_frames(rows, generator=generator, noise=noise, seed=seed, scale=scale)
        return out.view(len(clips), int(num_frames), *out.shape[1:])
