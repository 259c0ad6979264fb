"""Known-region sampling (video prediction, interpolation, inpainting): the mask builder and the one-launch blend the step-by-step
paths share with the fused chains (``latte_sample_loop_known``, ``latte_t2v_guided_ddim_loop_known``).  Not in the reference; the
scheme is the replacement method of Video Diffusion Models / RePaint."""
import numpy as np
import torch

from . import _lib
from ._lib import LatteError, check, load_library, ptr, stream_ptr


def known_mask(shape, frames=None, box=None):
    """The fp32 mask [B, F, H, W] of a clip of ``shape`` -- [B, F, H, W], or latents [B, F, C, H, W] whose channel axis is dropped: 1
    where the clip is known, 0 where it is generated.  ``frames``: indices of frames known entirely (negative ones count from the
    end); ``box`` = (y0, x0, y1, x1): the latent pixels [y0, y1) x [x0, x1) known in every frame.  Both: their union.  Host code."""
    shape = tuple(int(v) for v in shape)
    if len(shape) == 5:
        shape = shape[:2] + shape[3:]
    if len(shape) != 4 or min(shape) <= 0:
        raise LatteError(f"known_mask: shape must be [B, F, H, W] or [B, F, C, H, W], got {shape}")
    B, F, H, W = shape
    m = torch.zeros(B, F, H, W, dtype=torch.float32)
    for f in frames or ():
        f = int(f)
        if not -F <= f < F:
            raise LatteError(f"known_mask: frame {f} outside a clip of {F} frames")
        m[:, f] = 1.0
    if box is not None:
        if len(box) != 4:
            raise LatteError("known_mask: box must be (y0, x0, y1, x1)")
        y0, x0, y1, x1 = (int(v) for v in box)
        if not (0 <= y0 < y1 <= H and 0 <= x0 < x1 <= W):
            raise LatteError(f"known_mask: box {tuple(box)} is empty or outside {H} x {W} latent pixels")
        m[:, :, y0:y1, x0:x1] = 1.0
    return m


def level_coefs(abar):
    """The fp32 (sqrt(abar), sqrt(1 - abar)) of a level, narrowed as the engine narrows them (csrc/engine.cpp: level_coefs)."""
    ab = np.float32(abar)
    return float(np.sqrt(ab)), float(np.sqrt(np.float32(1.0) - ab))


def known_blend(x, known, mask, a, b, noise=None, seed=0, offset=0, frames_inner=False):
    """One ``latte_known_blend`` launch on ``x`` IN PLACE (fp32, contiguous, on the GPU) -> ``x``:
    ``x <- m == 1 ? kn : (m == 0 ? x : m kn + (1 - m) x)``, ``kn = b == 0 ? known : a known + b z``.  ``x`` / ``known`` / ``noise``:
    [B, F, C, H, W], or [B, C, F, H, W] with ``frames_inner`` (text-to-video); ``mask`` [B, F, H, W].  Without ``noise`` and with
    ``b != 0`` the kernel draws ``z`` itself from Philox at (``seed``, ``offset``)."""
    _lib.require_gpu()
    if x.dtype != torch.float32 or not x.is_contiguous() or x.dim() != 5:
        raise LatteError("known_blend: x must be a contiguous fp32 tensor of 5 dimensions")
    B, d1, d2, H, W = x.shape
    F, C = (d2, d1) if frames_inner else (d1, d2)
    kn = known.to(device=x.device, dtype=torch.float32).contiguous()
    mk = mask.to(device=x.device, dtype=torch.float32).contiguous()
    nz = None if noise is None else noise.to(device=x.device, dtype=torch.float32).contiguous()
    if kn.shape != x.shape or (nz is not None and nz.shape != x.shape):
        raise LatteError("known_blend: known and noise must have the shape of x")
    if mk.numel() != B * F * H * W:
        raise LatteError(f"known_blend: the mask must be [B, F, H, W] = {(B, F, H, W)}, got {tuple(mask.shape)}")
    with torch.cuda.device(x.device):
        check(load_library().latte_known_blend(ptr(x), ptr(kn), ptr(mk), ptr(nz), int(seed), int(offset), float(a), float(b), B, F, C, H * W,
                                               int(bool(frames_inner)), stream_ptr()))
    return x
