"""Clips longer than the model's ``num_frames``: overlapping temporal windows (temporal co-denoising as in Gen-L-Video / MultiDiffusion
along time).  The window set and the two launches the step-by-step paths share with the fused chains (``latte_sample_loop_windows``,
``latte_sample_plan_loop_windows``, ``latte_t2v_guided_*_loop_windows``).  Not in the reference; DESIGN.md section 4.10e."""
import ctypes

import torch

from . import _lib
from ._lib import LatteError, check, load_library, ptr, stream_ptr


def window_starts(total_frames, frames, stride):
    """The ascending first frames of the windows of a clip of ``total_frames`` >= ``frames`` at ``stride`` in 1 ... ``frames``:
    ``min(w * stride, total_frames - frames)`` for ``w`` in ``range(ceil((total_frames - frames) / stride) + 1)`` -- the last window
    is pulled back so that it ends with the clip.  ``latte_window_plan``: host only."""
    L, F, S = int(total_frames), int(frames), int(stride)
    starts = (ctypes.c_int * max(L, 1))()
    W = load_library().latte_window_plan(L, F, S, starts, None, max(L, 1))
    if W < 0:
        check(-W)
    return [int(starts[w]) for w in range(W)]


def window_counts(total_frames, frames, stride):
    """How many windows of ``window_starts`` cover each of the ``total_frames`` frames (every count >= 1).  Host only."""
    L = int(total_frames)
    counts = (ctypes.c_int * max(L, 1))()
    W = load_library().latte_window_plan(L, int(frames), int(stride), None, counts, 0)
    if W < 0:
        check(-W)
    return [int(counts[f]) for f in range(L)]


def _long_and_clip(name, t, frames, frames_inner):
    if t.dtype != torch.float32 or not t.is_contiguous() or t.dim() != 5:
        raise LatteError(f"{name}: the tensor must be a contiguous fp32 tensor of 5 dimensions")
    G, d1, d2, H, W = t.shape
    L, C = (d2, d1) if frames_inner else (d1, d2)
    shape = (lambda g, f: (g, C, f, H, W)) if frames_inner else (lambda g, f: (g, f, C, H, W))
    return G, L, C, H * W, shape


def window_gather(x, frames, stride, frames_inner=False):
    """One ``latte_window_gather`` launch: ``x`` [G, L, C, H, W] (fp32, contiguous, on the GPU) -> the clips [G * W, frames, C, H, W],
    clip ``g * W + w`` = ``x[g, s_w : s_w + frames]``.  ``frames_inner``: [G, C, L, H, W] -> [G * W, C, frames, H, W]
    (text-to-video)."""
    _lib.require_gpu()
    G, L, C, hw, shape = _long_and_clip("window_gather", x, frames, frames_inner)
    W = len(window_starts(L, frames, stride))
    clips = torch.empty(shape(G * W, int(frames)), device=x.device, dtype=torch.float32)
    with torch.cuda.device(x.device):
        check(load_library().latte_window_gather(ptr(x), ptr(clips), G, L, int(frames), int(stride), C, hw, int(bool(frames_inner)),
                                                 stream_ptr()))
    return clips


def window_merge(out, total_frames, stride, frames_inner=False):
    """One ``latte_window_merge`` launch: the model outputs of the clips ``out`` [G * W, F, C, H, W] (fp32, contiguous, on the GPU) ->
    [G, total_frames, C, H, W]: per frame the mean over the windows that cover it, summed in ascending window order; a frame of one
    window is copied.  ``frames_inner``: [G * W, C, F, H, W] -> [G, C, total_frames, H, W]."""
    _lib.require_gpu()
    GW, F, C, hw, shape = _long_and_clip("window_merge", out, None, frames_inner)
    W = len(window_starts(total_frames, F, stride))
    if GW % W:
        raise LatteError(f"window_merge: {GW} clips are no multiple of the {W} windows")
    merged = torch.empty(shape(GW // W, int(total_frames)), device=out.device, dtype=torch.float32)
    with torch.cuda.device(out.device):
        check(load_library().latte_window_merge(ptr(out), ptr(merged), GW // W, int(total_frames), F, int(stride), C, hw,
                                                int(bool(frames_inner)), stream_ptr()))
    return merged


def repeat_per_window(kwargs, batch, windows):
    """``kwargs`` with every tensor whose leading dimension is ``batch`` repeated per window (row ``g * W + w`` = row ``g``): what a
    model callable takes with the clips of ``window_gather``."""
    return {k: v.repeat_interleave(windows, dim=0) if torch.is_tensor(v) and v.dim() >= 1 and v.shape[0] == batch else v
            for k, v in kwargs.items()}
