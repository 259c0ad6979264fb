"""latte_amd.T5EncoderModel on the MI355X: every new kernel through its C-ABI hook against fp32 torch, the whole encoder against the
fp32 restatement (tests/t5_reference.py) and the transformers fixture (tests/golden/t5_tiny.npz), its exactness properties, and
text-to-video driven from a prompt string.

Bounds.  TOL = 1e-3 relative L2 is the project's parity contract.  The kernel bounds follow from the formats: a split pair carries
hi + lo / 2048 with |error| <= 2^-22 |x| (PAIR), a projection on pairs drops the lo . lo term (2^-22) and accumulates in fp32
(2^-24 sqrt(K) growth): 2e-6; plain f16 operands (attention: q, k, v, probabilities) round at 2^-11 = 4.9e-4 per operand, and the
unscaled scores (|s| of a few units here) turn a relative 2^-11 on s into that much absolute error in the exponent: 2e-3."""
import ctypes
import os

import numpy as np
import pytest
import torch

import latte_amd
import t5_reference as R
from _util import GOLDEN, rel_l2
from latte_amd._lib import c_void, load_library, ptr, stream_ptr
from latte_amd.random_init import t5_state_dict
from latte_amd.t5 import HashTokenizer

pytestmark = pytest.mark.gpu
TOL = 1e-3
PAIR = 2.0 ** -21


def _check(rc):
    assert rc == 0, load_library().latte_last_error()


def _pair(n, dev="cuda"):
    return torch.empty(n, dtype=torch.float16, device=dev), torch.empty(n, dtype=torch.float16, device=dev)


def _val(hi, lo):
    return hi.float() + lo.float() / 2048.0


def _pack(x, rows_pad=None):
    """fp32 [M, K] -> device pair, optionally padded with zero rows."""
    x = x.cuda().float().contiguous()
    if rows_pad and rows_pad > x.shape[0]:
        x = torch.cat([x, torch.zeros(rows_pad - x.shape[0], x.shape[1], device="cuda")]).contiguous()
    hi, lo = _pair(x.numel())
    _check(load_library().latte_debug_t5_pack(ptr(x), ptr(hi), ptr(lo), x.numel(), stream_ptr()))
    return hi.view(x.shape), lo.view(x.shape)


def test_embed_gather():
    g = torch.Generator().manual_seed(0)
    table = torch.randn(50, 64, generator=g)
    ids = torch.randint(0, 50, (37,), generator=g)
    out = torch.empty(37, 64, device="cuda")
    ids_d, table_d = ids.cuda(), table.cuda()
    _check(load_library().latte_debug_t5_embed(ptr(ids_d), ptr(table_d), ptr(out), 37, 64, 50, stream_ptr()))
    assert torch.equal(out.cpu(), table[ids])


@pytest.mark.parametrize("D", [256, 4096])
def test_rmsnorm(D):
    g = torch.Generator().manual_seed(1)
    x = torch.randn(9, D, generator=g)
    x[3] *= 3.0e5                       # beyond the f16 range (65504): the fp32 stream must not care
    x[4] *= 1.0e-3
    w = 1.0 + 0.2 * torch.randn(D, generator=g)
    want = R.rms_norm(x.double(), w.double(), 1e-6).float()
    xd, wd = x.cuda(), w.cuda()
    hi, lo = _pair(9 * D)
    _check(load_library().latte_debug_t5_rmsnorm(ptr(xd), ptr(wd), ptr(hi), ptr(lo), None, 9, D, 1e-6, stream_ptr()))
    got = _val(hi, lo).view(9, D)
    f32 = torch.empty(9, D, device="cuda")
    _check(load_library().latte_debug_t5_rmsnorm(ptr(xd), ptr(wd), None, None, ptr(f32), 9, D, 1e-6, stream_ptr()))
    for r in range(9):
        print(f"rmsnorm D={D} row {r}: pair {rel_l2(got[r], want[r]):.2e} fp32 {rel_l2(f32[r], want[r]):.2e}")
        assert rel_l2(f32[r], want[r]) < 1e-6 and rel_l2(got[r], want[r]) < 1e-6
    assert torch.equal(xd.cpu(), x)    # no slabs: the stream itself is untouched


@pytest.mark.parametrize("heads,max_len", [(4, 120), (64, 512)])
def test_bias_table(heads, max_len):
    rel = torch.randn(32, heads, generator=torch.Generator().manual_seed(2))
    table, rel_d = torch.empty(heads, 2 * max_len - 1, device="cuda"), rel.cuda()
    _check(load_library().latte_debug_t5_bias_table(ptr(rel_d), heads, 32, 128, max_len, ptr(table), stream_ptr()))
    want = R.position_bias(rel, max_len)                       # [h, i, j]
    i, j = torch.meshgrid(torch.arange(max_len), torch.arange(max_len), indexing="ij")
    assert torch.equal(table.cpu()[:, (j - i) + max_len - 1], want)


def test_bucket_function_host():
    lib = load_library()
    rel = torch.arange(-600, 601)
    got = torch.tensor([lib.latte_debug_t5_bucket(int(r), 32, 128) for r in rel])
    assert torch.equal(got, R.relative_position_bucket(rel))


@pytest.mark.parametrize("heads", [4, 64])
@pytest.mark.parametrize("L,valid", [(120, 1), (120, 37), (120, 120), (512, 512)])
def test_attention_bias_mask(heads, L, valid):
    g = torch.Generator().manual_seed(3)
    B, inner = 2, heads * 64
    qkv = torch.randn(B * L, 3 * inner, generator=g) * torch.tensor([0.35, 1.0, 1.0]).repeat_interleave(inner)
    qkv = qkv.to(torch.float16)
    rel = torch.randn(32, heads, generator=g)
    mask = torch.zeros(B, L)
    mask[0, :valid] = 1
    mask[1] = 1                                                # second sample: no padding
    table, rel_d, qkv_d, mask_d = torch.empty(heads, 2 * L - 1, device="cuda"), rel.cuda(), qkv.cuda(), mask.cuda()
    _check(load_library().latte_debug_t5_bias_table(ptr(rel_d), heads, 32, 128, L, ptr(table), stream_ptr()))
    hi, lo = _pair(B * L * inner)
    _check(load_library().latte_debug_t5_attention(ptr(qkv_d), ptr(table), ptr(mask_d), ptr(hi), ptr(lo), B, L, heads, L,
                                                  stream_ptr()))
    got = _val(hi, lo).view(B, L, heads, 64).cpu()
    q, k, v = (t.double().view(B, L, heads, 64).transpose(1, 2) for t in qkv.double().split(inner, dim=1))
    s = q @ k.transpose(-1, -2) + R.position_bias(rel, L).double()[None]
    s = s.masked_fill(mask[:, None, None, :] == 0, float("-inf"))
    want = (torch.softmax(s, -1) @ v).transpose(1, 2)
    e = rel_l2(got, want)
    print(f"t5 attention heads={heads} L={L} valid={valid}: {e:.3e}")
    assert e < 2e-3
    # a masked key has weight exactly 0: other values at the masked positions change nothing, bit for bit
    if valid < L:
        q2 = qkv.clone().view(B, L, -1)
        q2[0, valid:, inner:] = torch.randn(L - valid, 2 * inner, generator=g).to(torch.float16) * 7
        hi2, lo2 = _pair(B * L * inner)
        q2_d = q2.cuda()
        _check(load_library().latte_debug_t5_attention(ptr(q2_d), ptr(table), ptr(mask_d), ptr(hi2), ptr(lo2), B, L, heads, L,
                                                      stream_ptr()))
        assert torch.equal(hi2, hi) and torch.equal(lo2, lo)


def test_gated_activation():
    g = torch.Generator().manual_seed(4)
    M, F = 37, 640
    u = torch.randn(M, 2 * F, generator=g) * 3
    hi, lo = _pair(M * F)
    u_d = u.cuda()
    _check(load_library().latte_debug_t5_gated_act(ptr(u_d), ptr(hi), ptr(lo), M, F, stream_ptr()))
    want = (R.gelu_new(u[:, :F].double()) * u[:, F:].double())
    e = rel_l2(_val(hi, lo).view(M, F), want)
    print(f"gated activation: {e:.3e}")
    assert e < 1e-6


# the four projections of T5-v1.1-XXL: [q; k; v], o, [wi_0; wi_1], wo
@pytest.mark.parametrize("N,K", [(12288, 4096), (4096, 4096), (20480, 4096), (4096, 10240)])
@pytest.mark.parametrize("M", [120, 240])
def test_projection_xxl_shapes(M, N, K):
    g = torch.Generator().manual_seed(5)
    a = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) * K ** -0.5
    ah, al = _pack(a, rows_pad=256)
    wh, wl = _pack(w)
    splits = load_library().latte_debug_t5_proj_splits(N, K)
    assert splits >= 1
    slabs = torch.empty(splits * M * N, device="cuda")
    out = torch.zeros(M, N, device="cuda")
    _check(load_library().latte_debug_t5_proj(ptr(ah), ptr(al), ptr(wh), ptr(wl), ptr(slabs), ptr(out), M, N, K, stream_ptr()))
    want = (a.cuda().double() @ w.cuda().double().t())
    e = rel_l2(out, want)
    print(f"t5 projection M={M} N={N} K={K} splits={splits}: {e:.3e}")
    assert e < 2e-6
    # against plain f16 operands the pair must be far better (a dropped lo term would sit at ~3e-4)
    assert e < 0.05 * rel_l2(a.half().float().cuda().double() @ w.half().float().cuda().double().t(), want)


CASES = {"w256_d2": dict(d_model=256, num_heads=4, d_ff=640, num_layers=2, vocab_size=1000),
         "w512_d24": dict(d_model=512, num_heads=8, d_ff=1280, num_layers=24, vocab_size=1000),
         "xxl_d2": dict(d_model=4096, num_heads=64, d_ff=10240, num_layers=2, vocab_size=1000)}


def _inputs(vocab, B=2, L=120, seed=11):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(2, vocab, (B, L), generator=g)
    mask = torch.ones(B, L, dtype=torch.int64)
    mask[0, 37:] = 0                     # a padded tail
    if B > 1:
        mask[1, 1:] = 0                  # one valid token: what the negative prompt "" tokenises to
    ids[mask == 0] = 0
    return ids, mask


def _model(cfg, sd, **kw):
    return latte_amd.T5EncoderModel(cfg, **kw).load_state_dict(sd).to("cuda")


@pytest.mark.parametrize("name", list(CASES))
def test_encoder_matches_restatement(name):
    cfg = CASES[name]
    sd = t5_state_dict(3, **cfg)
    ids, mask = _inputs(cfg["vocab_size"])
    want = R.t5_encoder_forward(sd, ids, mask)
    m = _model(cfg, sd)
    out = m(ids.cuda(), attention_mask=mask.cuda())
    got = out.last_hidden_state
    assert out[0] is got and got.dtype == torch.float32 and tuple(got.shape) == (2, 120, cfg["d_model"])
    e = rel_l2(got, want)
    rows = ((got.cpu().double() - want.double()).norm(dim=-1) / want.double().norm(dim=-1)).max().item()
    emu = rel_l2(R.t5_encoder_forward(sd, ids, mask, emulate=R.T5_EMULATE_ENGINE), want) if name != "xxl_d2" else float("nan")
    print(f"t5 encoder {name}: rel-L2 {e:.3e} worst row {rows:.3e} (CPU emulation of the operand scheme: {emu:.3e})")
    assert e <= TOL
    # no mask == a mask of ones
    full = m(ids.cuda()).last_hidden_state
    assert torch.equal(full, m(ids.cuda(), attention_mask=torch.ones_like(mask).cuda()).last_hidden_state)
    assert rel_l2(full, R.t5_encoder_forward(sd, ids, None)) <= TOL


def test_encoder_matches_transformers_fixture():
    z = np.load(os.path.join(GOLDEN, "t5_tiny.npz"))
    import json
    cfg = json.loads(bytes(z["cfg_json"]).decode())
    sd = t5_state_dict(int(z["seed"]), **cfg)
    m = _model(cfg, sd, max_batch=int(z["ids"].shape[0]))
    got = m(torch.from_numpy(z["ids"]).cuda(), attention_mask=torch.from_numpy(z["mask"]).cuda()).last_hidden_state
    e = rel_l2(got, torch.from_numpy(z["out"]))
    print(f"t5 encoder vs transformers fixture: {e:.3e}")
    assert e <= TOL


def test_encoder_exactness_properties():
    cfg = CASES["w256_d2"]
    sd = t5_state_dict(3, **cfg)
    ids, mask = _inputs(cfg["vocab_size"])
    m = _model(cfg, sd)
    a = m(ids.cuda(), attention_mask=mask.cuda()).last_hidden_state.clone()
    assert torch.equal(a, m(ids.cuda(), attention_mask=mask.cuda()).last_hidden_state)          # repeated calls
    # batch rows are independent: swap the samples, replace the neighbour
    b = m(ids.flip(0).cuda(), attention_mask=mask.flip(0).cuda()).last_hidden_state
    assert torch.equal(b.flip(0), a)
    other, omask = _inputs(cfg["vocab_size"], seed=99)
    c = m(torch.stack([ids[0], other[0]]).cuda(), attention_mask=torch.stack([mask[0], omask[0]]).cuda()).last_hidden_state
    assert torch.equal(c[0], a[0])
    # B = 1 gives the rows of B = 2
    for r in range(2):
        one = m(ids[r:r + 1].cuda(), attention_mask=mask[r:r + 1].cuda()).last_hidden_state
        assert torch.equal(one[0], a[r])
    # ids at masked positions do not reach a valid row
    ids2 = ids.clone()
    ids2[mask == 0] = torch.randint(2, cfg["vocab_size"], (int((mask == 0).sum()),), generator=torch.Generator().manual_seed(5))
    d = m(ids2.cuda(), attention_mask=mask.cuda()).last_hidden_state
    valid = mask.bool()
    assert torch.equal(d.cpu()[valid], a.cpu()[valid])
    assert not torch.equal(d.cpu()[~valid], a.cpu()[~valid])
    # a shorter call than max_len
    s = m(ids[:, :40].cuda(), attention_mask=mask[:, :40].cuda()).last_hidden_state
    assert rel_l2(s, R.t5_encoder_forward(sd, ids[:, :40], mask[:, :40])) <= TOL
    with pytest.raises(latte_amd.LatteError):
        m(torch.zeros(3, 120, dtype=torch.int64).cuda())
    with pytest.raises(latte_amd.LatteError):
        m(ids)                                                  # CPU tensor


def test_pipeline_from_prompt_string():
    """prompt string -> stand-in tokenizer -> native T5 -> LatteT2V: the latents equal, bit for bit, those of the run that is handed
    the encoder's own outputs (masked as the reference masks them), and sit within the T2V tolerance of the run fed with the
    oracle's embeddings."""
    import json
    from latte_amd.schedulers import DDIMScheduler
    z = np.load(os.path.join(GOLDEN, "tiny_t2v.npz"))
    tcfg = json.loads(bytes(z["cfg_json"]).decode())
    tsd = {k[4:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd::")}
    tcfg.pop("norm_eps", None)
    tr = latte_amd.LatteT2V(compute_dtype="f16", **tcfg).load_state_dict(tsd)
    cfg = dict(d_model=tcfg["caption_channels"], num_heads=2, d_ff=128, num_layers=2, vocab_size=500)
    sd = t5_state_dict(7, **cfg)
    enc = _model(cfg, sd, max_batch=1)
    tok = HashTokenizer(cfg["vocab_size"])
    prompt, steps, scale = "A small Dog running on the beach", 3, 4.5
    lat = torch.randn(1, 4, tcfg["video_length"], tcfg["sample_size"], tcfg["sample_size"], generator=torch.Generator().manual_seed(2))
    pipe = latte_amd.LattePipeline(tokenizer=tok, text_encoder=enc, transformer=tr, scheduler=DDIMScheduler()).to("cuda")
    kw = dict(num_inference_steps=steps, guidance_scale=scale, latents=lat, output_type="latents",
              height=8 * tcfg["sample_size"], width=8 * tcfg["sample_size"], video_length=tcfg["video_length"])
    got = pipe(prompt=prompt, **kw).video
    # the same run from embeddings: prompt / "" through tokenizer and encoder by hand, masked as pipeline_latte.py:117-126, 255-262
    ti, ui = tok([prompt.lower().strip()], max_length=120), tok([""], max_length=120)
    keep = int(ti.attention_mask.sum())
    pe = enc(ti.input_ids.cuda(), attention_mask=ti.attention_mask.cuda())[0][:, :keep]
    ne = enc(ui.input_ids.cuda(), attention_mask=ui.attention_mask.cuda())[0][:, :keep]
    same = pipe(prompt_embeds=pe, negative_prompt_embeds=ne, **kw).video
    assert torch.equal(got, same)
    pe_o = R.t5_encoder_forward(sd, ti.input_ids, ti.attention_mask)[:, :keep]
    ne_o = R.t5_encoder_forward(sd, ui.input_ids, ui.attention_mask)[:, :keep]
    want = pipe(prompt_embeds=pe_o, negative_prompt_embeds=ne_o, **kw).video
    e = rel_l2(got, want)
    print(f"t2v latents, native T5 vs oracle embeddings: {e:.3e}")
    assert e < TOL
