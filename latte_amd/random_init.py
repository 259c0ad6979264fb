"""Random weights of the right shapes for plumbing runs and benchmarks (there are no checkpoints offline).

Not test infrastructure and not an oracle: these only FILL state dicts with reference-format keys (diffusers
``AutoencoderKL`` decoder and encoder keys of the sd-vae-ft architecture, ``LatteT2V`` keys of models/latte_t2v.py) so that
``bench.py`` and ``tools/*`` can time the device path.  ``Latte`` itself initialises like the reference
(latte.py:257-295); ``randomize_zero_init`` re-draws what that leaves at zero so outputs are not trivially 0.
"""
import math

import torch


def randomize_zero_init(model, std=0.02, seed=1):
    g = torch.Generator("cpu").manual_seed(seed)
    with torch.no_grad():
        for _, p in model.named_parameters():
            if p.requires_grad and float(p.detach().abs().max()) == 0.0:
                p.copy_(torch.randn(p.shape, generator=g) * std)
    return model


def _fill(keys, seed):
    g = torch.Generator("cpu").manual_seed(seed)
    sd = {}
    for k, shp in keys.items():
        if k.endswith("scale_shift_table"):
            sd[k] = torch.randn(shp, generator=g) / shp[-1] ** 0.5
        elif "norm" in k and k.endswith("weight"):
            sd[k] = 1.0 + 0.1 * torch.randn(shp, generator=g)
        elif k.endswith("bias"):
            sd[k] = 0.02 * torch.randn(shp, generator=g)
        else:
            sd[k] = torch.randn(shp, generator=g) / math.sqrt(max(math.prod(shp[1:]), 1))
    return sd


def vae_decoder_keys(block_out=(128, 256, 512, 512), layers=2, latent=4):
    """diffusers AutoencoderKL decoder half (post_quant_conv + decoder.*), sd-vae-ft layout."""
    ks = {"post_quant_conv.weight": (latent, latent, 1, 1), "post_quant_conv.bias": (latent,)}
    top = block_out[-1]
    ks["decoder.conv_in.weight"], ks["decoder.conv_in.bias"] = (top, latent, 3, 3), (top,)

    def resnet(p, cin, cout):
        ks[p + "norm1.weight"], ks[p + "norm1.bias"] = (cin,), (cin,)
        ks[p + "conv1.weight"], ks[p + "conv1.bias"] = (cout, cin, 3, 3), (cout,)
        ks[p + "norm2.weight"], ks[p + "norm2.bias"] = (cout,), (cout,)
        ks[p + "conv2.weight"], ks[p + "conv2.bias"] = (cout, cout, 3, 3), (cout,)
        if cin != cout:
            ks[p + "conv_shortcut.weight"], ks[p + "conv_shortcut.bias"] = (cout, cin, 1, 1), (cout,)

    resnet("decoder.mid_block.resnets.0.", top, top)
    a = "decoder.mid_block.attentions.0."
    ks[a + "group_norm.weight"], ks[a + "group_norm.bias"] = (top,), (top,)
    for n in ("to_q", "to_k", "to_v", "to_out.0"):
        ks[a + n + ".weight"], ks[a + n + ".bias"] = (top, top), (top,)
    resnet("decoder.mid_block.resnets.1.", top, top)
    rev, prev = list(reversed(block_out)), block_out[-1]
    for i, cout in enumerate(rev):
        for r in range(layers + 1):
            resnet(f"decoder.up_blocks.{i}.resnets.{r}.", prev if r == 0 else cout, cout)
        prev = cout
        if i != len(rev) - 1:
            ks[f"decoder.up_blocks.{i}.upsamplers.0.conv.weight"] = (cout, cout, 3, 3)
            ks[f"decoder.up_blocks.{i}.upsamplers.0.conv.bias"] = (cout,)
    ks["decoder.conv_norm_out.weight"], ks["decoder.conv_norm_out.bias"] = (block_out[0],), (block_out[0],)
    ks["decoder.conv_out.weight"], ks["decoder.conv_out.bias"] = (3, block_out[0], 3, 3), (3,)
    return ks


def vae_encoder_keys(block_out=(128, 256, 512, 512), layers=2, latent=4):
    """diffusers AutoencoderKL encoder half (encoder.* + quant_conv), sd-vae-ft layout (double_z: conv_out has 2 * latent channels)."""
    ks = {"encoder.conv_in.weight": (block_out[0], 3, 3, 3), "encoder.conv_in.bias": (block_out[0],)}

    def resnet(p, cin, cout):
        ks[p + "norm1.weight"], ks[p + "norm1.bias"] = (cin,), (cin,)
        ks[p + "conv1.weight"], ks[p + "conv1.bias"] = (cout, cin, 3, 3), (cout,)
        ks[p + "norm2.weight"], ks[p + "norm2.bias"] = (cout,), (cout,)
        ks[p + "conv2.weight"], ks[p + "conv2.bias"] = (cout, cout, 3, 3), (cout,)
        if cin != cout:
            ks[p + "conv_shortcut.weight"], ks[p + "conv_shortcut.bias"] = (cout, cin, 1, 1), (cout,)

    prev = block_out[0]
    for i, cout in enumerate(block_out):
        for r in range(layers):
            resnet(f"encoder.down_blocks.{i}.resnets.{r}.", prev if r == 0 else cout, cout)
        prev = cout
        if i != len(block_out) - 1:
            ks[f"encoder.down_blocks.{i}.downsamplers.0.conv.weight"] = (cout, cout, 3, 3)
            ks[f"encoder.down_blocks.{i}.downsamplers.0.conv.bias"] = (cout,)
    top = block_out[-1]
    resnet("encoder.mid_block.resnets.0.", top, top)
    a = "encoder.mid_block.attentions.0."
    ks[a + "group_norm.weight"], ks[a + "group_norm.bias"] = (top,), (top,)
    for n in ("to_q", "to_k", "to_v", "to_out.0"):
        ks[a + n + ".weight"], ks[a + n + ".bias"] = (top, top), (top,)
    resnet("encoder.mid_block.resnets.1.", top, top)
    ks["encoder.conv_norm_out.weight"], ks["encoder.conv_norm_out.bias"] = (top,), (top,)
    ks["encoder.conv_out.weight"], ks["encoder.conv_out.bias"] = (2 * latent, top, 3, 3), (2 * latent,)
    ks["quant_conv.weight"], ks["quant_conv.bias"] = (2 * latent, 2 * latent, 1, 1), (2 * latent,)
    return ks


def vae_encoder_state_dict(seed=0):
    return _fill(vae_encoder_keys(), seed)


def vae_decoder_state_dict(seed=0):
    return _fill(vae_decoder_keys(), seed)


def vae_temporal_decoder_keys():
    """diffusers AutoencoderKLTemporalDecoder decoder keys: the SD-VAE decoder's with every resnet split into
    ``spatial_res_block`` / ``temporal_res_block`` (Conv3d (3,1,1)) / ``time_mixer.mix_factor``, no post_quant_conv, plus
    ``decoder.time_conv_out``."""
    ks = {}
    base = vae_decoder_keys()
    for k, shp in base.items():
        if k.startswith("post_quant_conv"):
            continue
        if ".resnets." in k:
            head, tail = k.rsplit(".", 2)[0], ".".join(k.rsplit(".", 2)[1:])      # "...resnets.N", "conv1.weight"
            ks[f"{head}.spatial_res_block.{tail}"] = shp
            if not tail.startswith("conv_shortcut"):
                c = base[f"{head}.norm2.weight"][0]                               # the temporal block works on out_channels
                ks[f"{head}.temporal_res_block.{tail}"] = (c, c, 3, 1, 1) if tail.endswith("weight") and tail.startswith("conv") else (c,)
            ks[f"{head}.time_mixer.mix_factor"] = (1,)
        else:
            ks[k] = shp
    ks["decoder.time_conv_out.weight"], ks["decoder.time_conv_out.bias"] = (3, 3, 3, 1, 1), (3,)
    return ks


def vae_temporal_decoder_state_dict(seed=0):
    sd = _fill(vae_temporal_decoder_keys(), seed)
    for k in sd:
        if k.endswith("mix_factor"):
            sd[k] = torch.zeros(1)            # AlphaBlender(alpha = 0.0): sigmoid(0) = 0.5
    return sd


def t2v_keys(num_attention_heads=16, attention_head_dim=72, in_channels=4, out_channels=8, num_layers=28, patch_size=2,
             cross_attention_dim=1152, caption_channels=4096, **unused):
    """State-dict keys of LatteT2V (models/latte_t2v.py) in the Latte-1 configuration."""
    D, p = num_attention_heads * attention_head_dim, patch_size
    ks = {"scale_shift_table": (2, D), "pos_embed.proj.weight": (D, in_channels, p, p), "pos_embed.proj.bias": (D,)}

    def attn(pre, kv):
        for n, i in (("to_q", D), ("to_k", kv), ("to_v", kv), ("to_out.0", D)):
            ks[pre + n + ".weight"], ks[pre + n + ".bias"] = (D, i), (D,)

    for kind, cross in (("transformer_blocks", True), ("temporal_transformer_blocks", False)):
        for i in range(num_layers):
            b = f"{kind}.{i}."
            ks[b + "scale_shift_table"] = (6, D)
            attn(b + "attn1.", D)
            if cross:
                attn(b + "attn2.", cross_attention_dim)
            ks[b + "ff.net.0.proj.weight"], ks[b + "ff.net.0.proj.bias"] = (4 * D, D), (4 * D,)
            ks[b + "ff.net.2.weight"], ks[b + "ff.net.2.bias"] = (D, 4 * D), (D,)
    ks["proj_out.weight"], ks["proj_out.bias"] = (p * p * out_channels, D), (p * p * out_channels,)
    e = "adaln_single.emb.timestep_embedder."
    ks[e + "linear_1.weight"], ks[e + "linear_1.bias"] = (D, 256), (D,)
    ks[e + "linear_2.weight"], ks[e + "linear_2.bias"] = (D, D), (D,)
    ks["adaln_single.linear.weight"], ks["adaln_single.linear.bias"] = (6 * D, D), (6 * D,)
    ks["caption_projection.linear_1.weight"], ks["caption_projection.linear_1.bias"] = (D, caption_channels), (D,)
    ks["caption_projection.linear_2.weight"], ks["caption_projection.linear_2.bias"] = (D, D), (D,)
    return ks


def t2v_state_dict(seed=0, **config):
    return _fill(t2v_keys(**config), seed)


def t5_keys(d_model=4096, d_kv=64, num_heads=64, d_ff=10240, num_layers=24, vocab_size=32128, relative_attention_num_buckets=32,
            **unused):
    """State-dict keys of ``transformers.T5EncoderModel`` (T5 v1.1, gated-gelu); the defaults are Latte-1's text_encoder (XXL).
    ``encoder.embed_tokens.weight`` is the tied duplicate of ``shared.weight`` that ``state_dict()`` also lists."""
    inner = num_heads * d_kv
    ks = {"shared.weight": (vocab_size, d_model), "encoder.embed_tokens.weight": (vocab_size, d_model)}
    for i in range(num_layers):
        a, f = f"encoder.block.{i}.layer.0.", f"encoder.block.{i}.layer.1."
        for n in "qkv":
            ks[a + f"SelfAttention.{n}.weight"] = (inner, d_model)
        ks[a + "SelfAttention.o.weight"] = (d_model, inner)
        if i == 0:
            ks[a + "SelfAttention.relative_attention_bias.weight"] = (relative_attention_num_buckets, num_heads)
        ks[a + "layer_norm.weight"] = (d_model,)
        ks[f + "DenseReluDense.wi_0.weight"], ks[f + "DenseReluDense.wi_1.weight"] = (d_ff, d_model), (d_ff, d_model)
        ks[f + "DenseReluDense.wo.weight"] = (d_model, d_ff)
        ks[f + "layer_norm.weight"] = (d_model,)
    ks["encoder.final_layer_norm.weight"] = (d_model,)
    return ks


def t5_state_dict(seed=0, **config):
    """``transformers``' own init scales (T5PreTrainedModel._init_weights, factor 1), except: ``relative_attention_bias`` has unit
    variance (stock: d_model^-0.5) and the norm weights are 1 + 0.2 randn (stock: exactly 1), so that a wrong bias index or a
    dropped norm weight changes the output by far more than any parity bound."""
    ks = t5_keys(**config)
    d_model = ks["shared.weight"][1]
    d_kv = config.get("d_kv", 64)
    g = torch.Generator("cpu").manual_seed(seed)
    sd = {}
    for k, shp in ks.items():
        if k == "encoder.embed_tokens.weight":
            sd[k] = sd["shared.weight"]
            continue
        r = torch.randn(shp, generator=g)
        if k.endswith("layer_norm.weight"):
            sd[k] = 1.0 + 0.2 * r
        elif k == "shared.weight" or k.endswith("relative_attention_bias.weight"):
            sd[k] = r
        elif k.endswith("SelfAttention.q.weight"):
            sd[k] = r * (d_model * d_kv) ** -0.5
        else:                                   # k, v, wi_0, wi_1: d_model^-0.5; o: inner^-0.5; wo: d_ff^-0.5 (all = fan_in^-0.5)
            sd[k] = r * shp[1] ** -0.5
    return sd
