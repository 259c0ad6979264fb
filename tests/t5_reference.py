"""fp32 restatement of ``transformers.T5EncoderModel`` (T5 v1.1, gated-gelu) in plain torch: the oracle of
``latte_amd.T5EncoderModel`` where ``transformers`` is not installed.  tests/test_t5_host.py pins it to the live
``transformers`` model (1e-5) and to the committed fixture tests/golden/t5_tiny.npz, which holds ``transformers``' own outputs.

``emulate`` restates the engine's operand rounding on the CPU so that the operand choice is reproducible without a GPU.  It
is a set of operand names, each rounded to f16 (fp32 accumulation everywhere, as on the MFMA):

  "w"     every projection weight
  "act"   the activation operand of every projection (RMSNorm output, attention output, gated activation)
  "qk"    q and k in the score product
  "pv"    the softmax probabilities and v in the context product

``T5_EMULATE_ALL`` is a plain-f16 engine; ``T5_EMULATE_ENGINE`` is what the engine runs for ``compute_dtype="f16"``: every
projection operand, weights included, is a split f16 pair (exact to ~2^-22, i.e. not rounded at this scale), so only the
attention operands round.
"""
import math

import torch

T5_EMULATE_ALL = frozenset(("w", "act", "qk", "pv"))
T5_EMULATE_ENGINE = frozenset(("qk", "pv"))


def relative_position_bucket(rel, num_buckets=32, max_distance=128):
    """Bidirectional bucket of rel = key position - query position (int64 tensor): modeling_t5.py T5Attention._relative_position_bucket."""
    nb = num_buckets // 2
    out = (rel > 0).to(torch.long) * nb
    n = rel.abs()
    max_exact = nb // 2
    large = max_exact + (torch.log(n.float() / max_exact) / math.log(max_distance / max_exact) * (nb - max_exact)).to(torch.long)
    large = torch.min(large, torch.full_like(large, nb - 1))
    return out + torch.where(n < max_exact, n, large)


def position_bias(table, L, num_buckets=32, max_distance=128):
    """[heads, L, L] from the [num_buckets, heads] table of block 0."""
    pos = torch.arange(L)
    bucket = relative_position_bucket(pos[None, :] - pos[:, None], num_buckets, max_distance)
    return table.float()[bucket].permute(2, 0, 1)


def _r(x, on):
    return x.to(torch.float16).float() if on else x


def rms_norm(x, w, eps):
    return w * (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps))


def gelu_new(x):
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x.pow(3))))


def t5_encoder_forward(sd, input_ids, attention_mask=None, num_heads=None, d_kv=64, num_buckets=32, max_distance=128, eps=1e-6,
                       emulate=frozenset()):
    """last_hidden_state [B, L, d_model] (fp32) of the ``transformers`` state dict ``sd`` on int64 ids [B, L]."""
    sd = {k: v.float() for k, v in sd.items()}
    B, L = input_ids.shape
    num_layers = 1 + max(int(k.split(".")[2]) for k in sd if k.startswith("encoder.block."))
    num_heads = num_heads or sd["encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"].shape[1]
    ew, ea, eqk, epv = ("w" in emulate), ("act" in emulate), ("qk" in emulate), ("pv" in emulate)
    mask = torch.ones(B, L) if attention_mask is None else attention_mask.float()
    x = sd["shared.weight"][input_ids]
    bias = position_bias(sd["encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"], L, num_buckets, max_distance)
    bias = bias[None] + ((1.0 - mask) * torch.finfo(torch.float32).min)[:, None, None, :]
    for i in range(num_layers):
        p = f"encoder.block.{i}.layer."
        n = _r(rms_norm(x, sd[p + "0.layer_norm.weight"], eps), ea)
        q, k, v = (F_linear(n, _r(sd[p + f"0.SelfAttention.{c}.weight"], ew)).view(B, L, num_heads, d_kv).transpose(1, 2) for c in "qkv")
        s = _r(q, eqk) @ _r(k, eqk).transpose(-1, -2) + bias
        ctx = _r(torch.softmax(s, -1), epv) @ _r(v, epv)
        ctx = ctx.transpose(1, 2).reshape(B, L, num_heads * d_kv)
        x = x + F_linear(_r(ctx, ea), _r(sd[p + "0.SelfAttention.o.weight"], ew))
        n = _r(rms_norm(x, sd[p + "1.layer_norm.weight"], eps), ea)
        h = gelu_new(F_linear(n, _r(sd[p + "1.DenseReluDense.wi_0.weight"], ew))) * F_linear(n, _r(sd[p + "1.DenseReluDense.wi_1.weight"], ew))
        x = x + F_linear(_r(h, ea), _r(sd[p + "1.DenseReluDense.wo.weight"], ew))
    return rms_norm(x, sd["encoder.final_layer_norm.weight"], eps)


def F_linear(x, w):
    return x @ w.t()


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm())
