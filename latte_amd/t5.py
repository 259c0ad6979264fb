"""Host-side mirror of ``transformers.T5EncoderModel`` for the call sites of the reference's text-to-video sampling
(sample/sample_t2x.py:36, sample/pipeline_latte.py:207,244):

    text_encoder = T5EncoderModel.from_pretrained(path, subfolder="text_encoder").to(device)
    prompt_embeds = text_encoder(input_ids, attention_mask=attention_mask)[0]

The encoder runs on the MI355X engine (``latte_t5_*`` in include/latte_amd.h): T5 v1.1 (gated-gelu), fp32 residual stream,
split f16 operand pairs in every projection, f16 attention operands.  Weights keep their ``transformers`` state-dict names.
There is no CPU fallback.
"""
import ctypes
import json
import os
from types import SimpleNamespace

import torch

from . import _lib
from ._lib import LatteError, check, load_library, ptr, stream_ptr
from .random_init import t5_keys

_CONFIG_KEYS = ("d_model", "d_kv", "num_heads", "d_ff", "num_layers", "vocab_size", "relative_attention_num_buckets",
                "relative_attention_max_distance", "layer_norm_epsilon", "feed_forward_proj")
_DEFAULTS = dict(d_model=4096, d_kv=64, num_heads=64, d_ff=10240, num_layers=24, vocab_size=32128, relative_attention_num_buckets=32,
                 relative_attention_max_distance=128, layer_norm_epsilon=1e-6, feed_forward_proj="gated-gelu")
_TIED = ("shared.weight", "encoder.embed_tokens.weight")


class BaseModelOutput:
    """What ``transformers`` returns: ``.last_hidden_state``, also reachable as ``[0]``."""

    def __init__(self, last_hidden_state):
        self.last_hidden_state = last_hidden_state

    def __getitem__(self, i):
        return (self.last_hidden_state,)[i]


class T5EncoderModel:
    """T5 v1.1 encoder on the HIP engine; the defaults are Latte-1's ``text_encoder`` (T5-v1.1-XXL).

    ``config`` is a mapping / object with the ``transformers`` T5Config fields, or pass them as keyword arguments.  Only
    ``compute_dtype="f16"`` is offered: 1e-3 relative L2 against fp32 at depth 24 needs more than 11 mantissa bits in the
    projection operands, which the engine carries as split f16 pairs; a bf16 variant was not built.
    ``max_batch`` x ``max_len`` sizes the workspace (``max_len`` <= 512)."""

    def __init__(self, config=None, compute_dtype="f16", max_batch=2, max_len=120, **kwargs):
        cfg = dict(_DEFAULTS)
        if config is not None:
            src = config if isinstance(config, dict) else vars(config)
            cfg.update({k: src[k] for k in _CONFIG_KEYS if k in src})
        unknown = set(kwargs) - set(_CONFIG_KEYS)
        if unknown:
            raise LatteError(f"latte_amd.T5EncoderModel: unknown configuration field(s) {sorted(unknown)}")
        cfg.update(kwargs)
        if cfg["feed_forward_proj"] != "gated-gelu":
            raise LatteError("latte_amd.T5EncoderModel implements T5 v1.1 only (feed_forward_proj 'gated-gelu'), got "
                             f"{cfg['feed_forward_proj']!r}")
        if compute_dtype not in ("f16", "fp16", "float16"):
            raise LatteError(f"latte_amd.T5EncoderModel runs f16 operand pairs only (class docstring): compute_dtype={compute_dtype!r}")
        if cfg["d_kv"] != 64 or cfg["d_model"] % 64 or cfg["d_ff"] % 64:
            raise LatteError("latte_amd.T5EncoderModel needs d_kv == 64 and d_model, d_ff multiples of 64")
        if not 1 <= max_len <= 512:
            raise LatteError("latte_amd.T5EncoderModel: max_len must be in [1, 512]")
        self.config = SimpleNamespace(**cfg)
        self.compute_dtype, self.max_batch, self.max_len = "f16", int(max_batch), int(max_len)
        self._shapes = t5_keys(**cfg)
        self._sd = {}
        self._device = torch.device("cpu")
        self._h, self._key, self._synced = None, None, False

    # ------------------------------------------------------------------ transformers-style loading
    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, subfolder="text_encoder", **kw):
        root = pretrained_model_name_or_path if subfolder is None else os.path.join(pretrained_model_name_or_path, subfolder)
        cfg_path = os.path.join(root, "config.json")
        if not os.path.exists(cfg_path):
            raise LatteError(f"no config.json under {root}")
        with open(cfg_path) as f:
            cfg = json.load(f)
        model = cls({k: cfg[k] for k in _CONFIG_KEYS if k in cfg},
                    **{k: v for k, v in kw.items() if k in ("compute_dtype", "max_batch", "max_len")})
        from safetensors.torch import load_file
        index, single = os.path.join(root, "model.safetensors.index.json"), os.path.join(root, "model.safetensors")
        if os.path.exists(index):
            with open(index) as f:
                files = sorted(set(json.load(f)["weight_map"].values()))
        elif os.path.exists(single):
            files = ["model.safetensors"]
        else:
            raise LatteError(f"no model.safetensors / model.safetensors.index.json under {root}")
        sd = {}
        for name in files:
            sd.update(load_file(os.path.join(root, name)))
        return model.load_state_dict(sd)

    def load_state_dict(self, state_dict, strict=True):
        sd = {}
        for k, v in state_dict.items():
            if k not in self._shapes:
                raise LatteError(f'Unexpected key(s) in state_dict: "{k}"')
            if tuple(v.shape) != tuple(self._shapes[k]):
                raise LatteError(f"size mismatch for {k}: got shape {tuple(v.shape)}, expected {tuple(self._shapes[k])}")
            sd[k] = v.detach()
        if not any(k in sd for k in _TIED):
            raise LatteError(f'Missing key(s) in state_dict: "{_TIED[0]}"')
        for k in self._shapes:
            if k not in sd and k not in _TIED:
                raise LatteError(f'Missing key(s) in state_dict: "{k}"')
        self._sd = sd
        self._synced = False
        return self

    def state_dict(self):
        sd = dict(self._sd)
        for a, b in (_TIED, _TIED[::-1]):           # safetensors drops one name of a tied pair; transformers lists both
            if a in sd and b not in sd:
                sd[b] = sd[a]
        return sd

    def to(self, *args, **kwargs):
        self._device = _lib.to_device(args, kwargs, self._device,
                                      "latte_amd.T5EncoderModel runs f16 operand pairs only (class docstring)")
        return self                                  # the engine state follows the device of the first call (_ensure)

    def eval(self):
        return self

    def requires_grad_(self, flag=False):
        return self

    @property
    def dtype(self):
        return torch.float16

    @property
    def device(self):
        return self._device

    def __del__(self):
        try:
            if self._h is not None:
                load_library().latte_t5_destroy(self._h)
        except Exception:
            pass

    # ------------------------------------------------------------------ engine plumbing
    def _ensure(self, device):
        lib = load_library()
        if self._h is None or self._key != device:
            if self._h is not None:
                lib.latte_t5_destroy(self._h)
                self._h = None
            c = self.config
            cfg = _lib.T5Config(c.d_model, c.d_kv, c.num_heads, c.d_ff, c.num_layers, c.vocab_size, c.relative_attention_num_buckets,
                                c.relative_attention_max_distance, float(c.layer_norm_epsilon), _lib.DTYPES["f16"])
            h = ctypes.c_void_p()
            check(lib.latte_t5_create(ctypes.byref(cfg), self.max_batch, self.max_len, ctypes.byref(h)))
            self._h, self._key, self._synced = h, device, False
        if not self._synced:
            if not self._sd:
                raise LatteError("latte_amd.T5EncoderModel: no weights loaded (load_state_dict / from_pretrained)")
            done = False
            for k, v in self._sd.items():
                if k in _TIED:
                    if done:
                        continue                       # the tied duplicate: one upload fills the table
                    done = True
                dev = v.to(device=device, dtype=torch.float32).contiguous()
                shape = (ctypes.c_int64 * dev.dim())(*dev.shape)
                check(lib.latte_t5_load_weight(self._h, k.encode(), ptr(dev), shape, dev.dim(), stream_ptr()))
                torch.cuda.current_stream().synchronize()   # `dev` is a temporary: its pack must finish before it is freed
            check(lib.latte_t5_check_weights(self._h))
            self._synced = True

    def __call__(self, input_ids, attention_mask=None, **unused):
        _lib.require_gpu()
        if not isinstance(input_ids, torch.Tensor) or input_ids.device.type != "cuda":
            raise LatteError("latte_amd.T5EncoderModel runs on the MI355X only: input_ids must be a CUDA/HIP tensor (no CPU fallback)")
        if input_ids.dim() != 2:
            raise LatteError("input_ids must be [batch, length]")
        B, L = input_ids.shape
        if B > self.max_batch or L > self.max_len:
            raise LatteError(f"input_ids {B} x {L} exceeds max_batch x max_len = {self.max_batch} x {self.max_len}")
        device = input_ids.device
        with torch.cuda.device(device):
            self._ensure(device)
            ids = input_ids.to(torch.int64).contiguous()
            mask = None
            if attention_mask is not None:
                if tuple(attention_mask.shape) != (B, L):
                    raise LatteError("attention_mask must have the shape of input_ids")
                mask = attention_mask.to(device=device, dtype=torch.float32).contiguous()
            out = torch.empty(B, L, self.config.d_model, device=device, dtype=torch.float32)
            check(load_library().latte_t5_forward(self._h, ptr(ids), ptr(mask), B, L, ptr(out), stream_ptr()))
        return BaseModelOutput(out)

    forward = __call__


class HashTokenizer:
    """Deterministic stand-in for ``T5Tokenizer`` where no SentencePiece model is at hand (tools/sample_t2x.py --random, tests): every
    whitespace-separated token maps to ``2 + sha256(token) mod (vocab_size - 2)``, an EOS (1) closes the sequence and padding (0) fills
    it to ``max_length``.  Same call signature and result fields as the tokenizer call of pipeline_latte.py:187-194.  It does not
    produce T5's ids: it only drives the encoder from a prompt string reproducibly."""
    pad_token_id, eos_token_id = 0, 1

    def __init__(self, vocab_size=32128):
        self.vocab_size = int(vocab_size)

    def token_id(self, token):
        import hashlib
        return 2 + int.from_bytes(hashlib.sha256(token.encode("utf-8")).digest()[:8], "little") % (self.vocab_size - 2)

    def __call__(self, text, padding="max_length", max_length=120, truncation=True, return_attention_mask=True, add_special_tokens=True,
                 return_tensors="pt", **unused):
        if isinstance(text, str):
            text = [text]
        ids = torch.full((len(text), max_length), self.pad_token_id, dtype=torch.int64)
        mask = torch.zeros(len(text), max_length, dtype=torch.int64)
        for r, t in enumerate(text):
            row = [self.token_id(w) for w in t.split()]
            if add_special_tokens:
                row = row[:max_length - 1] + [self.eos_token_id]
            row = row[:max_length]
            ids[r, :len(row)] = torch.tensor(row, dtype=torch.int64)
            mask[r, :len(row)] = 1
        return SimpleNamespace(input_ids=ids, attention_mask=mask)
