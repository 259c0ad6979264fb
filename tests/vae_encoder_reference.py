"""fp32 CPU restatement of the SD-VAE ENCODER -- test infrastructure for tests/test_vae_encoder.py.

PARITY WITH REAL DIFFUSERS IS UNPINNED.  Like the decoder oracle (oracle/vae_oracle.py), this restates the published architecture
of diffusers 0.24.0's ``AutoencoderKL.encode`` for the sd-vae-ft config in plain torch ops; diffusers is not installed anywhere this
project runs, so agreement with it is unverified.  The resnet and attention blocks are the decoder oracle's own (imported).

Structure followed (diffusers 0.24.0):
  AutoencoderKL.encode          : x -> Encoder -> quant_conv (1x1, 8 -> 8) -> DiagonalGaussianDistribution(moments)
  vae.Encoder.forward           : conv_in (3 -> 128) -> down_blocks[0..3] -> mid_block -> conv_norm_out -> SiLU -> conv_out (512 -> 8)
  DownEncoderBlock2D            : 2 x ResnetBlock2D (+ Downsample2D on blocks 0..2)
  Downsample2D(use_conv, pad 0) : F.pad(x, (0, 1, 0, 1)) then conv3x3 with stride 2 and no padding
  DiagonalGaussianDistribution  : mean, logvar = moments.chunk(2, 1); logvar.clamp(-30, 20); std = exp(0.5 logvar); sample = mean + std eps
"""
import torch
import torch.nn.functional as F

from latte_amd.random_init import vae_encoder_keys  # noqa: F401  (the key table the tests compare against)
from oracle.vae_oracle import BLOCK_OUT, EPS, GROUPS, LAYERS_PER_BLOCK, _attention, _resnet


def downsample(x, w, b):
    """Downsample2D(use_conv=True, padding=0): the asymmetric zero pad, then a 3x3 stride-2 convolution."""
    return F.conv2d(F.pad(x, (0, 1, 0, 1), mode="constant", value=0), w, b, stride=2)


def encode_moments(sd, x, block_out=BLOCK_OUT, layers=LAYERS_PER_BLOCK, trace=None):
    """x: [N, 3, H, W] fp32 in [-1, 1] -> moments [N, 8, H/8, W/8] (DiagonalGaussianDistribution.parameters).
    trace: optional list receiving the activation after conv_in, every down-block resnet and down-sampler, each mid-block member and
    the moments (the stage order of latte_debug_vae_encode_trace)."""
    def t(v):
        if trace is not None:
            trace.append(v.clone())
        return v
    with torch.no_grad():
        h = t(F.conv2d(x, sd["encoder.conv_in.weight"], sd["encoder.conv_in.bias"], padding=1))
        for i in range(len(block_out)):
            for r in range(layers):
                h = t(_resnet(sd, f"encoder.down_blocks.{i}.resnets.{r}.", h))
            if i != len(block_out) - 1:
                p = f"encoder.down_blocks.{i}.downsamplers.0.conv."
                h = t(downsample(h, sd[p + "weight"], sd[p + "bias"]))
        h = t(_resnet(sd, "encoder.mid_block.resnets.0.", h))
        h = t(_attention(sd, "encoder.mid_block.attentions.0.", h))
        h = t(_resnet(sd, "encoder.mid_block.resnets.1.", h))
        h = F.silu(F.group_norm(h, GROUPS, sd["encoder.conv_norm_out.weight"], sd["encoder.conv_norm_out.bias"], EPS))
        h = F.conv2d(h, sd["encoder.conv_out.weight"], sd["encoder.conv_out.bias"], padding=1)
        return t(F.conv2d(h, sd["quant_conv.weight"], sd["quant_conv.bias"]))


def posterior(moments):
    """(mean, logvar clamped, std, var) of DiagonalGaussianDistribution."""
    mean, logvar = torch.chunk(moments, 2, dim=1)
    logvar = torch.clamp(logvar, -30.0, 20.0)
    return mean, logvar, torch.exp(0.5 * logvar), torch.exp(logvar)


def sample(moments, noise):
    mean, _, std, _ = posterior(moments)
    return mean + std * noise
