"""The host side of latte_amd.T5EncoderModel, without a GPU: the fp32 restatement (tests/t5_reference.py) pinned to live
``transformers`` and to the committed transformers fixture, the key set, the state-dict shim and the stand-in tokenizer."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import latte_amd
import t5_reference as R
from _util import GOLDEN
from latte_amd.random_init import t5_keys, t5_state_dict
from latte_amd.t5 import HashTokenizer

HAVE_TRANSFORMERS = importlib.util.find_spec("transformers") is not None
needs_transformers = pytest.mark.skipif(not HAVE_TRANSFORMERS, reason="transformers is not installed")
TINY = dict(d_model=128, num_heads=4, d_ff=256, num_layers=2, vocab_size=200)


def _hf(cfg):
    from transformers import T5Config, T5EncoderModel
    c = dict(d_kv=64, relative_attention_num_buckets=32, relative_attention_max_distance=128)
    c.update(cfg)
    return T5EncoderModel(T5Config(feed_forward_proj="gated-gelu", layer_norm_epsilon=1e-6, dropout_rate=0.0, **c)).eval()


def _inputs(vocab, B=3, L=120, seed=1):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(2, vocab, (B, L), generator=g)
    mask = torch.ones(B, L, dtype=torch.int64)
    mask[1, 37:] = 0                    # a padded tail
    mask[2, 1:] = 0                     # one valid token: the negative prompt ""
    ids[mask == 0] = 0
    return ids, mask


@needs_transformers
@pytest.mark.parametrize("cfg", [dict(d_model=128, num_heads=4, d_ff=256, num_layers=2, vocab_size=200),
                                 dict(d_model=256, num_heads=2, d_ff=640, num_layers=4, vocab_size=300),
                                 dict(d_model=192, num_heads=5, d_ff=320, num_layers=3, vocab_size=100,
                                      relative_attention_num_buckets=16, relative_attention_max_distance=64)],
                         ids=["w128_d2", "w256_d4", "w192_d3_b16"])
def test_restatement_matches_transformers(cfg):
    sd = t5_state_dict(2, **cfg)
    model = _hf(cfg)
    model.load_state_dict(sd)
    ids, mask = _inputs(cfg["vocab_size"])
    with torch.no_grad():
        want = model(input_ids=ids, attention_mask=mask).last_hidden_state
        want_nomask = model(input_ids=ids).last_hidden_state
    kw = dict(num_buckets=cfg.get("relative_attention_num_buckets", 32), max_distance=cfg.get("relative_attention_max_distance", 128))
    e = R.rel_l2(R.t5_encoder_forward(sd, ids, mask, **kw), want)
    e2 = R.rel_l2(R.t5_encoder_forward(sd, ids, None, **kw), want_nomask)
    print(f"restatement vs transformers: {e:.2e} (masked) {e2:.2e} (no mask)")
    assert e < 1e-5 and e2 < 1e-5


@needs_transformers
@pytest.mark.parametrize("nb,md", [(32, 128), (16, 64)])
def test_bucket_function_matches_transformers(nb, md):
    from transformers.models.t5.modeling_t5 import T5Attention
    rel = torch.arange(-600, 601)
    want = T5Attention._relative_position_bucket(rel, bidirectional=True, num_buckets=nb, max_distance=md)
    assert torch.equal(R.relative_position_bucket(rel, nb, md), want)


def test_bucket_function_of_the_engine(lib):
    """The engine builds its bias table from a host-side bucket function (fp32 arithmetic as in the reference)."""
    rel = torch.arange(-600, 601)
    for nb, md in ((32, 128), (16, 64)):
        got = torch.tensor([lib.latte_debug_t5_bucket(int(r), nb, md) for r in rel])
        assert torch.equal(got, R.relative_position_bucket(rel, nb, md))


def _fixture():
    z = np.load(os.path.join(GOLDEN, "t5_tiny.npz"))
    return z, json.loads(bytes(z["cfg_json"]).decode())


def test_restatement_matches_transformers_fixture():
    """Carries the pin to machines without transformers: the fixture's outputs are transformers' own (tools/make_t5_golden.py)."""
    z, cfg = _fixture()
    assert os.path.getsize(os.path.join(GOLDEN, "t5_tiny.npz")) < 512 * 1024
    sd = t5_state_dict(int(z["seed"]), **cfg)
    total = float(sum(v.double().abs().sum() for k, v in sorted(sd.items()) if k != "encoder.embed_tokens.weight"))
    assert abs(total - float(z["weight_abs_sum"])) <= 1e-9 * float(z["weight_abs_sum"])
    ids, mask = torch.from_numpy(z["ids"]), torch.from_numpy(z["mask"])
    assert int(mask[1].sum()) == 37 and int(mask[2].sum()) == 1
    e = R.rel_l2(R.t5_encoder_forward(sd, ids, mask), torch.from_numpy(z["out"]))
    print(f"restatement vs transformers fixture: {e:.2e}")
    assert e < 1e-5


def test_emulation_switch_orders_the_operand_schemes():
    """The operand choice on the CPU: every operand in f16 costs several times what the engine's scheme does (DESIGN.md quotes depth 24)."""
    cfg = dict(d_model=256, num_heads=4, d_ff=640, num_layers=2, vocab_size=300)
    sd = t5_state_dict(3, **cfg)
    ids, mask = _inputs(300)
    ref = R.t5_encoder_forward(sd, ids, mask)
    plain = R.rel_l2(R.t5_encoder_forward(sd, ids, mask, emulate=R.T5_EMULATE_ALL), ref)
    engine = R.rel_l2(R.t5_encoder_forward(sd, ids, mask, emulate=R.T5_EMULATE_ENGINE), ref)
    print(f"emulation at width 256, depth 2: all-f16 {plain:.2e}, engine scheme {engine:.2e}")
    assert 0 < engine < plain < 1e-3


@needs_transformers
def test_keys_match_transformers():
    model = _hf(TINY)
    want = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    assert t5_keys(**TINY) == want
    sd = t5_state_dict(0, **TINY)
    assert {k: tuple(v.shape) for k, v in sd.items()} == want
    assert sd["encoder.embed_tokens.weight"] is sd["shared.weight"]
    rb = sd["encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"]
    assert 0.8 < float(rb.std()) < 1.2                                    # unit variance, not d_model^-0.5
    ln = sd["encoder.block.1.layer.1.layer_norm.weight"]
    assert 0.1 < float(ln.std()) < 0.3 and abs(float(ln.mean()) - 1) < 0.1
    # T5-v1.1-XXL, shapes only
    from transformers import T5Config, T5EncoderModel
    with torch.device("meta"):
        xxl = T5EncoderModel(T5Config(d_model=4096, d_kv=64, num_heads=64, d_ff=10240, num_layers=24, vocab_size=32128,
                                      feed_forward_proj="gated-gelu"))
    want = {k: tuple(v.shape) for k, v in xxl.state_dict().items()}
    assert t5_keys() == want


def test_xxl_key_count_and_parameter_total():
    ks = t5_keys()
    assert len(ks) == 2 + 24 * 9 + 1 + 1
    total = sum(int(np.prod(s)) for k, s in ks.items() if k != "encoder.embed_tokens.weight")
    assert total == 4_762_310_656                                          # T5-v1.1-XXL encoder: 4.76 G parameters
    assert latte_amd.T5EncoderModel().config.d_model == 4096              # the defaults are Latte-1's text_encoder


def test_state_dict_shim():
    sd = t5_state_dict(0, **TINY)
    m = latte_amd.T5EncoderModel(TINY)
    assert m.load_state_dict(sd) is m and set(m.state_dict()) == set(sd)
    assert m.eval() is m and m.dtype == torch.float16 and m.config.num_layers == 2
    one = {k: v for k, v in sd.items() if k != "encoder.embed_tokens.weight"}       # what a safetensors file holds
    assert set(latte_amd.T5EncoderModel(TINY).load_state_dict(one).state_dict()) == set(sd)
    other = {k: v for k, v in sd.items() if k != "shared.weight"}
    assert set(latte_amd.T5EncoderModel(TINY).load_state_dict(other).state_dict()) == set(sd)
    with pytest.raises(latte_amd.LatteError, match="Missing"):
        m.load_state_dict({k: v for k, v in sd.items() if "final_layer_norm" not in k})
    with pytest.raises(latte_amd.LatteError, match="Missing"):
        m.load_state_dict({k: v for k, v in sd.items() if k not in ("shared.weight", "encoder.embed_tokens.weight")})
    with pytest.raises(latte_amd.LatteError, match="Unexpected"):
        m.load_state_dict(dict(sd, **{"decoder.final_layer_norm.weight": torch.zeros(128)}))
    with pytest.raises(latte_amd.LatteError, match="size mismatch"):
        m.load_state_dict(dict(sd, **{"encoder.final_layer_norm.weight": torch.zeros(64)}))
    with pytest.raises(latte_amd.LatteError):
        latte_amd.T5EncoderModel(TINY, compute_dtype="bf16")
    with pytest.raises(latte_amd.LatteError):
        latte_amd.T5EncoderModel(dict(TINY, feed_forward_proj="relu"))
    with pytest.raises(latte_amd.LatteError):
        latte_amd.T5EncoderModel(dict(TINY, d_kv=32))
    with pytest.raises(latte_amd.LatteError):
        m.to(torch.bfloat16)
    with pytest.raises(latte_amd.LatteError):                               # CPU tensor / no GPU: no fallback
        m(torch.zeros(1, 8, dtype=torch.int64))


@pytest.mark.parametrize("sharded", [False, True])
def test_from_pretrained_directory(tmp_path, sharded):
    from safetensors.torch import save_file
    sd = t5_state_dict(1, **TINY)
    root = tmp_path / "text_encoder"
    root.mkdir()
    cfg = dict(TINY, d_kv=64, relative_attention_num_buckets=32, relative_attention_max_distance=128, layer_norm_epsilon=1e-6,
               feed_forward_proj="gated-gelu", model_type="t5", architectures=["T5EncoderModel"])
    (root / "config.json").write_text(json.dumps(cfg))
    flat = {k: v.contiguous() for k, v in sd.items() if k != "encoder.embed_tokens.weight"}     # tied duplicate: not in the file
    if sharded:
        keys = sorted(flat)
        parts = {"model-00001-of-00002.safetensors": keys[::2], "model-00002-of-00002.safetensors": keys[1::2]}
        for name, ks in parts.items():
            save_file({k: flat[k] for k in ks}, str(root / name))
        (root / "model.safetensors.index.json").write_text(json.dumps({"metadata": {}, "weight_map": {k: n for n, ks in parts.items() for k in ks}}))
    else:
        save_file(flat, str(root / "model.safetensors"))
    m = latte_amd.T5EncoderModel.from_pretrained(str(tmp_path), subfolder="text_encoder", max_len=64)
    assert m.max_len == 64 and m.config.d_ff == 256
    got = m.state_dict()
    assert set(got) == set(sd) and all(torch.equal(got[k], sd[k]) for k in sd)
    with pytest.raises(latte_amd.LatteError):
        latte_amd.T5EncoderModel.from_pretrained(str(tmp_path), subfolder="nope")


def test_standin_tokenizer():
    tok = HashTokenizer(32128)
    a = tok(["a dog running on the beach", ""], padding="max_length", max_length=120, truncation=True, return_attention_mask=True,
            add_special_tokens=True, return_tensors="pt")
    b = HashTokenizer(32128)(["a dog running on the beach", ""], max_length=120)
    assert torch.equal(a.input_ids, b.input_ids) and torch.equal(a.attention_mask, b.attention_mask)
    assert a.input_ids.dtype == torch.int64 and tuple(a.input_ids.shape) == (2, 120)
    assert a.attention_mask.sum(1).tolist() == [7, 1]                       # six words + EOS; "" is the EOS alone
    assert a.input_ids[0, 6] == 1 and a.input_ids[1, 0] == 1 and int(a.input_ids[0, 7:].abs().sum()) == 0
    assert int(a.input_ids.max()) < 32128 and int(a.input_ids[0, :6].min()) >= 2
    assert a.input_ids[0, 0] == 2 + int.from_bytes(__import__("hashlib").sha256(b"a").digest()[:8], "little") % 32126   # stable across runs
    long = tok([" ".join(["w%d" % i for i in range(300)])], max_length=120)
    assert int(long.attention_mask.sum()) == 120 and long.input_ids[0, 119] == 1
    # the pipeline lower-cases and strips before the tokenizer (pipeline_latte.py:182): the ids do not depend on the prompt's case
    from latte_amd.schedulers import DDIMScheduler
    seen = []

    def spy(texts, **kw):
        seen.append(tok(texts, **kw))
        return seen[-1]

    pipe = latte_amd.LattePipeline(tokenizer=spy, text_encoder=lambda ids, attention_mask=None: (torch.zeros(ids.shape[0], ids.shape[1], 8),),
                                   transformer=object(), scheduler=DDIMScheduler())
    pipe.encode_prompt(["  A Dog Running On The BEACH \n"], negative_prompt="", device="cpu")
    assert torch.equal(seen[0].input_ids, a.input_ids[:1]) and torch.equal(seen[1].input_ids, a.input_ids[1:])
