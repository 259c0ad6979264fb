"""The weight store behind latte_engine / latte_t2v / latte_vae / latte_t5 (latte_amd/csrc/weight_store.h) through the C ABI: the
ordered key lists against tests/golden/engine_keys.json (recorded from the per-engine slot tables this store replaced), every error
string and return code of the load frame, the optional-key and tied-group rules, the host-pointer staging path and the reload
invalidation of latte_engine.

Sizes.  The smallest configurations the creators accept: the Latte of test_training_step.py (depth 2, hidden 128), tests/golden's tiny
T2V and tiny T5, and the VAE at latent 16 / image 128 with max_frames 1 (latent_size % 16 and image_size % 128 are enforced by
latte_vae_create*, so latent 8 / image 64 cannot be created; a key list does not depend on the size)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import latte_amd
from _util import GOLDEN
from latte_amd import _lib
from latte_amd._lib import c_void, load_library, ptr, stream_ptr
from latte_amd.random_init import (randomize_zero_init, t5_state_dict, vae_decoder_keys, vae_encoder_keys,
                                   vae_temporal_decoder_keys)

pytestmark = pytest.mark.gpu
OK, ERR_INVALID, ERR_STATE = 0, 1, 3
LATTE_KW = dict(depth=2, hidden_size=128, patch_size=2, num_heads=2, input_size=8, num_frames=16)
LOAD_PREFIX = {"engine": "load_tensor", "t2v": "t2v_load_tensor", "vae": "vae_load_tensor"}


def _err():
    return load_library().latte_last_error().decode()


class _Engine:
    """A raw handle of one family ("engine" | "t2v" | "vae" | "t5"), destroyed with the object."""

    def __init__(self, family, handle):
        self.family, self.h, self.lib = family, handle, load_library()

    def fn(self, name):
        return getattr(self.lib, f"latte_{self.family}_{name}")

    def keys(self):
        return [self.fn("key")(self.h, i).decode() for i in range(self.fn("num_keys")(self.h))]

    def load(self, key, t, numel=None, on_device=1):
        return self.fn("load_tensor")(self.h, key.encode(), ptr(t), t.numel() if numel is None else numel, on_device, stream_ptr())

    def load_all(self, sd, on_device=1, skip=()):
        for k in self.keys():
            if k in skip:
                continue
            t = sd[k].detach().to(device="cuda" if on_device else "cpu", dtype=torch.float32).contiguous()
            assert self.load(k, t, on_device=on_device) == OK, _err()
        torch.cuda.synchronize()

    def check(self):
        return self.fn("check_weights")(self.h)

    def __del__(self):
        try:
            self.fn("destroy")(self.h)
        except Exception:
            pass


def _latte_module(extras=1, seed=1):
    return randomize_zero_init(latte_amd.Latte(extras=extras, **LATTE_KW), seed=seed)


def _latte_engine(module, max_batch=2):
    h = c_void()
    assert load_library().latte_engine_create(module.engine_config("f16"), max_batch, h) == OK, _err()
    return _Engine("engine", h)


def _t2v_fixture():
    z = np.load(os.path.join(GOLDEN, "tiny_t2v.npz"))
    c = json.loads(bytes(z["cfg_json"]).decode())
    sd = {k[4:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd::")}
    return c, sd


def _t2v_engine():
    c, sd = _t2v_fixture()
    cfg = _lib.T2VConfig(c["num_attention_heads"], c["attention_head_dim"], c["in_channels"], c["out_channels"], c["num_layers"],
                         c["sample_size"], c["patch_size"], c["cross_attention_dim"], c["caption_channels"], c["video_length"], 120,
                         _lib.DTYPES["f16"])
    h = c_void()
    assert load_library().latte_t2v_create(cfg, 2, h) == OK, _err()
    return _Engine("t2v", h), sd


def _vae_engine(mode):
    create = {"decoder": "latte_vae_create", "temporal": "latte_vae_create_temporal", "encoder": "latte_vae_create_encoder"}[mode]
    h = c_void()
    assert getattr(load_library(), create)(128 if mode == "encoder" else 16, 1, _lib.DTYPES["f16"], h) == OK, _err()
    return _Engine("vae", h)


def _t5_fixture():
    z = np.load(os.path.join(GOLDEN, "t5_tiny.npz"))
    cfg = json.loads(bytes(z["cfg_json"]).decode())
    return cfg, t5_state_dict(int(z["seed"]), **cfg)


def _t5_engine():
    c, sd = _t5_fixture()
    cfg = _lib.T5Config(c["d_model"], c["d_kv"], c["num_heads"], c["d_ff"], c["num_layers"], c["vocab_size"],
                        c["relative_attention_num_buckets"], c["relative_attention_max_distance"], 1e-6, _lib.DTYPES["f16"])
    h = c_void()
    assert load_library().latte_t5_create(ctypes.byref(cfg), 2, 120, ctypes.byref(h)) == OK, _err()
    return _Engine("t5", h), sd


def _t5_load(e, key, t, shape=None):
    t = t.detach().to(device="cuda", dtype=torch.float32).contiguous()
    shape = tuple(t.shape) if shape is None else shape
    rc = e.lib.latte_t5_load_weight(e.h, key.encode(), ptr(t), (ctypes.c_int64 * len(shape))(*shape), len(shape), stream_ptr())
    torch.cuda.synchronize()   # `t` is a temporary
    return rc


def engine_key_lists():
    """{name: ordered key list} of every engine configuration in tests/golden/engine_keys.json."""
    out = {f"latte_extras{x}": _latte_engine(latte_amd.Latte(extras=x, **LATTE_KW)).keys() for x in (1, 2, 78)}
    out["t2v_tiny"] = _t2v_engine()[0].keys()
    for mode in ("decoder", "temporal", "encoder"):
        out["vae_" + mode] = _vae_engine(mode).keys()
    out["t5_tiny"] = _t5_engine()[0].keys()
    return out


def test_key_lists_match_the_recorded_order():
    with open(os.path.join(GOLDEN, "engine_keys.json")) as f:
        want = json.load(f)
    got = engine_key_lists()
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name] == want[name], name


def _family_case(family):
    """-> (engine, {key: tensor of the expected numel}) with every key of the engine present."""
    if family == "engine":
        m = _latte_module()
        return _latte_engine(m), m.state_dict()
    if family == "t2v":
        return _t2v_engine()
    shapes = vae_decoder_keys()
    return _vae_engine("decoder"), {k: torch.zeros(s, device="cuda") for k, s in shapes.items()}


@pytest.mark.parametrize("family", ["engine", "t2v", "vae"])
def test_load_frame_errors_and_check_weights(family):
    e, sd = _family_case(family)
    keys, prefix = e.keys(), LOAD_PREFIX[family]
    dummy = torch.zeros(4, device="cuda")
    assert e.check() == ERR_STATE
    assert _err() == f'Missing key(s) in state_dict: "{keys[0]}"'
    assert e.load("no.such.key", dummy) == ERR_INVALID
    assert _err() == f"{prefix}: unexpected key 'no.such.key'"
    n = sd[keys[0]].numel()
    assert e.load(keys[0], dummy, numel=n + 1) == ERR_INVALID
    assert _err() == f"{prefix}: size mismatch for '{keys[0]}': got {n + 1}, expected {n}"
    assert e.fn("load_tensor")(e.h, None, ptr(dummy), 4, 1, stream_ptr()) == ERR_INVALID
    assert _err() == f"{prefix}: null argument"
    assert e.check() == ERR_STATE                       # the refused loads marked nothing
    assert _err() == f'Missing key(s) in state_dict: "{keys[0]}"'
    e.load_all(sd, skip=(keys[-1],))
    assert e.check() == ERR_STATE
    assert _err() == f'Missing key(s) in state_dict: "{keys[-1]}"'
    e.load_all(sd)
    assert e.check() == OK


def test_t2v_optional_key():
    e, sd = _t2v_engine()
    k = "caption_projection.y_embedding"
    assert k in e.keys()
    e.load_all(sd, skip=(k,))
    assert e.check() == OK                              # not required
    assert e.load(k, torch.zeros(4, device="cuda"), numel=3) == OK   # accepted with any numel
    assert e.check() == OK


@pytest.mark.parametrize("loaded", ["shared.weight", "encoder.embed_tokens.weight"])
def test_t5_tied_group(loaded):
    e, sd = _t5_engine()
    tied = ("shared.weight", "encoder.embed_tokens.weight")
    assert e.keys()[:2] == list(tied)
    assert e.check() == ERR_STATE
    assert _err() == 'Missing key(s) in state_dict: "shared.weight"'
    for k in e.keys():
        if k not in tied:
            assert _t5_load(e, k, sd[k]) == OK, _err()
    assert e.check() == ERR_STATE                       # neither member of the group yet
    assert _err() == 'Missing key(s) in state_dict: "shared.weight"'
    assert _t5_load(e, loaded, sd["shared.weight"]) == OK, _err()
    assert e.check() == OK


def test_t5_shape_rule():
    e, sd = _t5_engine()
    k = "encoder.block.0.layer.1.DenseReluDense.wo.weight"
    w = sd[k]                                           # [d_model, d_ff] = [128, 256]
    assert _t5_load(e, k, w, shape=(w.shape[1], w.shape[0])) == ERR_INVALID   # right numel, wrong shape
    assert _err() == f"t5_load_weight: size mismatch for '{k}': got shape (256, 128), expected (128, 256)"
    assert _t5_load(e, k, w, shape=(w.numel(),)) == ERR_INVALID
    assert _err() == f"t5_load_weight: size mismatch for '{k}': got shape (32768), expected (128, 256)"
    assert _t5_load(e, "no.such.key", w) == ERR_INVALID
    assert _err() == "t5_load_weight: unexpected key 'no.such.key'"
    assert _t5_load(e, k, w) == OK, _err()


def _inputs(B):
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, 16, 4, 8, 8, generator=g).cuda()
    return x, torch.full((B,), 500, dtype=torch.int64).cuda()


def _forward(e, x, t, guided=False):
    out = torch.empty(x.shape[0], 16, 8, 8, 8, device="cuda")
    if guided:
        rc = e.lib.latte_forward_with_cfg(e.h, ptr(x), ptr(t), None, x.shape[0], 7.0, ptr(out), stream_ptr())
    else:
        rc = e.lib.latte_forward(e.h, ptr(x), ptr(t), None, x.shape[0], ptr(out), stream_ptr())
    assert rc == OK, _err()
    torch.cuda.synchronize()
    return out


def test_host_pointer_loads_match_device_loads():
    """The staging path (on_device = 0: host source -> staging buffer -> pack, one synchronize per tensor) against device sources."""
    m = _latte_module()
    sd = m.state_dict()
    host, dev = _latte_engine(m), _latte_engine(m)
    host.load_all(sd, on_device=0)
    dev.load_all(sd, on_device=1)
    assert host.check() == OK and dev.check() == OK
    x, t = _inputs(1)
    a, b = _forward(host, x, t), _forward(dev, x, t)
    assert torch.isfinite(a).all() and float(a.abs().max()) > 0
    assert torch.equal(a, b)


def test_reload_invalidates_the_derived_weight_copies():
    """A guided forward builds the split-operand copies of the block weights ([W | W] of fc1 at this shape); reloading fc1 must
    rebuild them behind the new conversion (latte_engine: split_w_ready, load_event)."""
    m = _latte_module()
    sd = dict(m.state_dict())
    k = "blocks.0.mlp.fc1.weight"
    e = _latte_engine(m)
    e.load_all(sd)
    x, t = _inputs(2)
    first = _forward(e, x, t, guided=True)
    active = ctypes.c_int64(0)
    assert e.lib.latte_engine_get_option(e.h, b"guided_split_active", ctypes.byref(active)) == OK
    assert active.value != 0                            # a derived copy is in use: a stale one would show below
    w2 = (sd[k].detach() + 0.5 * torch.randn(sd[k].shape, generator=torch.Generator().manual_seed(9))).cuda().contiguous()
    assert e.load(k, w2) == OK, _err()
    second = _forward(e, x, t, guided=True)
    assert not torch.equal(first, second)
    fresh = _latte_engine(m)
    fresh.load_all({**sd, k: w2})
    assert torch.equal(second, _forward(fresh, x, t, guided=True))
