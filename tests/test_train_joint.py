"""Joint image-video training on the engine (LatteTrainer(use_image_num=N), latte_trainer_*_joint): a joint micro-batch runs as the
plain video step plus a spatial-only image pass whose gradient writers add (include/latte_amd.h).  The oracle is the fp32 restatement
of LatteIMG.forward + training_losses (tests/joint_reference.py, pinned to the reference by tests/test_joint_reference.py).

Gradient bound: every tensor's relative L2 error against the restatement stays below max(GTOL[dtype], 1.25 e_plain), where e_plain is
the worst tensor of the UNCHANGED video-only forward_backward on the same weights and the case's video frames against
oracle.train_oracle.loss_and_grads, measured in the same test.  GTOL is an empirical figure of another weight draw
(tests/test_train_accum.py:33-37), so the plain path on these weights sets the margin, not the joint path; 1.25 is the factor
tests/test_training_step.py uses between two paths of one step.  Terms: the training-step tests' 1e-4."""
import functools
import json
import os
import types

import pytest
import torch

from oracle import diffusion_oracle as do
from oracle import latte_oracle as lo
from oracle import train_oracle as to
from test_training_step import GTOL, rel

import joint_reference as jr

pytestmark = pytest.mark.gpu

MUST_COMPARE = ("t_embedder.mlp.0.weight", "t_embedder.mlp.0.bias", "t_embedder.mlp.2.weight", "t_embedder.mlp.2.bias",
                "blocks.0.adaLN_modulation.1.weight", "blocks.0.adaLN_modulation.1.bias", "blocks.1.adaLN_modulation.1.weight",
                "blocks.1.adaLN_modulation.1.bias", "final_layer.linear.weight", "final_layer.linear.bias",
                "final_layer.adaLN_modulation.1.weight", "final_layer.adaLN_modulation.1.bias")


def model_kw(extras=2, **kw):
    return dict(jr.J_MODEL, extras=extras, **kw)


@functools.lru_cache(maxsize=None)
def case(extras=2, images=jr.J_IMAGES, batch=3, **kw):
    """Weights, inputs and both oracles' results of one configuration, computed once: the restatement on the joint micro-batch and
    oracle.train_oracle on its video frames."""
    mkw = model_kw(extras, **kw)
    cfg, sd, x0, noise, t, y, yi, drop, idrop = jr.joint_inputs(mkw, images=images, batch=batch)
    s = do.Schedule("")
    terms, out, grads = jr.joint_loss_and_grads(sd, cfg, s, x0, t, noise, y, yi, drop, idrop, images=images)
    Fr = cfg.num_frames
    _, _, grads_video = to.loss_and_grads(sd, cfg, s, x0[:, :Fr], t, noise[:, :Fr], y, drop)
    return mkw, cfg, sd, (x0, noise, t, y, yi, drop, idrop), terms, out, grads, grads_video


def trainer(mkw, sd, max_batch, images, dtype="f16", fuse_small=1, **kw):
    import latte_amd
    model = latte_amd.Latte(**mkw)
    model.load_state_dict(sd)
    kw.setdefault("start_clip_iter", 10 ** 9)
    tr = latte_amd.LatteTrainer(model.to("cuda"), latte_amd.create_diffusion(""), max_batch=max_batch, compute_dtype=dtype,
                                use_image_num=images, **kw)
    if not fuse_small:
        tr.set_option("fuse_small", 0)
    return tr, model


def grads_of(tr):
    torch.cuda.synchronize()
    return {k: v.cpu().clone() for k, v in tr.grad_dict().items()}


def record(key, worst, e_plain, bound):
    """The measured worst tensors into the JSON file LATTE_JOINT_PARITY_JSON names (profiles/train_joint_parity.json was written so);
    nothing is written when it is unset."""
    path = os.environ.get("LATTE_JOINT_PARITY_JSON")
    if not path:
        return
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    tab = json.load(open(path)) if os.path.exists(path) else {}
    tab[key] = {"worst_tensor": max(worst, key=worst.get), "worst_rel_l2": max(worst.values()),
                "median_rel_l2": sorted(worst.values())[len(worst) // 2], "plain_video_step_worst_rel_l2": e_plain, "bound": bound}
    json.dump(tab, open(path, "w"), indent=1, sort_keys=True)


def check_parity(label, c, images, dtype="f16", fuse_small=1):
    """The joint step of case ``c`` against the restatement, bounded through the plain video step on the same weights."""
    mkw, cfg, sd, (x0, noise, t, y, yi, drop, idrop), terms, out_ref, grads_ref, grads_video = c
    B, Fr = x0.shape[0], cfg.num_frames
    plain, _ = trainer(mkw, sd, B, 0, dtype, fuse_small)
    plain.forward_backward(x0[:, :Fr], t, noise[:, :Fr], y, drop)
    got_plain = grads_of(plain)
    e_plain = max(rel(got_plain[k], grads_video[k]) for k in grads_video)
    del plain
    bound = max(GTOL[dtype], 1.25 * e_plain)
    tr, _ = trainer(mkw, sd, B, images, dtype, fuse_small)
    out = tr.forward_backward(x0, t, noise, y, drop, return_model_out=True, y_image=yi, image_drop_mask=idrop)
    got = grads_of(tr)
    for k in ("loss", "mse", "vb"):
        print(label, k, out[k].cpu().tolist(), terms[k].tolist())
        assert rel(out[k].cpu(), terms[k]) < 1e-4, (k, out[k].cpu(), terms[k])
    assert set(got) == set(grads_ref)
    worst = {k: rel(got[k], grads_ref[k]) for k in grads_ref}
    record(label, worst, e_plain, bound)
    print(label, "worst gradient tensor", max(worst, key=worst.get), max(worst.values()), "plain video step", e_plain, "bound", bound)
    for k in MUST_COMPARE + (("y_embedder.embedding_table.weight",) if cfg.extras == 2 else ()):
        assert k in worst, k
        print("   ", k, worst[k])
    print("    model output", rel(out["model_out"].cpu(), out_ref))
    # the model output through half operands: the bound of the gradients it feeds
    assert rel(out["model_out"].cpu(), out_ref) < bound
    bad = {k: round(v, 6) for k, v in worst.items() if not v < bound}
    assert not bad, (bad, bound)
    return tr, got


# ------------------------------------------------------------------------------------------------ 1. parity on fixture J
@pytest.mark.parametrize("extras", [2, 1])
@pytest.mark.parametrize("fuse_small", [1, 0])
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_joint_step_matches_the_restatement_on_fixture_j(dtype, fuse_small, extras):
    c = case(extras)
    assert (c[3][0].shape[0] * jr.J_IMAGES * 64) % 128 != 0          # the image pass walks the padded tail of the 128-row tiles
    tr, got = check_parity(f"J::extras{extras}::fuse_small{fuse_small}::{dtype}", c, jr.J_IMAGES, dtype, fuse_small)
    if extras == 2:   # rows of the label table: 3 only images carry, 5 (null) a dropped video label and dropped image labels; 2 was dropped
        gy = got["y_embedder.embedding_table.weight"]
        assert all(float(gy[r].abs().max()) > 0 for r in (0, 1, 3, 4, 5))


# ------------------------------------------------------------------------------------------------ 2. images never reach a temporal block
def test_image_frames_do_not_reach_the_temporal_blocks():
    mkw, cfg, sd, (x0, noise, t, y, yi, drop, idrop), *_ = case(2)
    Fr = cfg.num_frames
    tr, _ = trainer(mkw, sd, 3, jr.J_IMAGES)
    tr.forward_backward(x0, t, noise, y, drop, y_image=yi, image_drop_mask=idrop)
    a = grads_of(tr)
    g = torch.Generator("cpu").manual_seed(99)
    x1, n1 = x0.clone(), noise.clone()
    x1[:, Fr:] = (torch.randn(x0[:, Fr:].shape, generator=g) * 0.6).clamp(-1.0, 1.0)
    n1[:, Fr:] = torch.randn(noise[:, Fr:].shape, generator=g)
    tr.forward_backward(x1, t, n1, y, drop, y_image=(yi + 1) % cfg.num_classes, image_drop_mask=~idrop)
    b = grads_of(tr)
    temporal = [k for k in a if k.startswith(("blocks.1.", "blocks.3."))]
    assert len(temporal) == 20
    for k in temporal:
        assert float(a[k].abs().max()) > 0.0, k
        assert torch.equal(a[k], b[k]), k
    assert not torch.equal(a["blocks.0.attn.qkv.weight"], b["blocks.0.attn.qkv.weight"])      # the spatial blocks did see them


# ------------------------------------------------------------------------------------------------ 3. the old path is untouched
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_plain_step_of_a_joint_trainer_is_bit_identical(dtype):
    mkw, cfg, sd, (x0, noise, t, y, yi, drop, idrop), *_ = case(2)
    Fr = cfg.num_frames
    res = []
    for images in (0, jr.J_IMAGES):
        tr, model = trainer(mkw, sd, 3, images, dtype)
        if images:                                             # a joint step first: nothing of it may stay behind
            tr.forward_backward(x0, t, noise, y, drop, y_image=yi, image_drop_mask=idrop)
        out = tr.forward_backward(x0[:, :Fr], t, noise[:, :Fr], y, drop)
        g = grads_of(tr)
        terms = {k: v.cpu().clone() for k, v in out.items()}
        norm = float(tr.optimizer_step())
        torch.cuda.synchronize()
        res.append((g, terms, norm, tr.params.cpu().clone(), tr.ema.cpu().clone(), tr.exp_avg_sq.cpu().clone()))
        del tr, model
    (g0, t0, n0, p0, e0, v0), (g1, t1, n1, p1, e1, v1) = res
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k
    for k in t0:
        assert torch.equal(t0[k], t1[k]), k
    assert n0 == n1 and torch.equal(p0, p1) and torch.equal(e0, e1) and torch.equal(v0, v1)


# ------------------------------------------------------------------------------------------------ 4. capacity edge
def test_as_many_images_as_frames_and_what_is_refused():
    import latte_amd
    c = case(2, images=4, batch=2)
    check_parity("J::N=F=4", c, 4)
    mkw, cfg, sd, (x0, noise, t, y, yi, drop, idrop), *_ = c
    with pytest.raises(latte_amd.LatteError):
        trainer(mkw, sd, 2, 5)                                 # use_image_num > num_frames
    lib = latte_amd._lib.load_library()
    model = latte_amd.Latte(**mkw).to("cuda")
    h = latte_amd._lib.c_void()
    assert lib.latte_trainer_create_joint(model.engine_config("f16"), 2, 5, h) != 0      # the engine refuses it too
    tr, _ = trainer(mkw, sd, 2, 4)
    with pytest.raises(latte_amd.LatteError):
        tr.forward_backward(x0[:, :7], t, noise[:, :7], y, drop, y_image=yi[:, :3])      # 7 frames: neither F nor F + N
    with pytest.raises(latte_amd.LatteError):
        tr.forward_backward(x0, t, noise, y, drop)                                       # class-conditional: y_image missing
    with pytest.raises(latte_amd.LatteError):
        tr.forward_backward(x0, t, noise, y, drop, y_image=yi[:, :3])                    # [B, 3] labels for 4 images
    small = model_kw(2, input_size=8)                                                    # T = 16: no multiple of 64
    with pytest.raises(latte_amd.LatteError):
        trainer(small, lo.init_state_dict(lo.LatteConfig(**small), seed=1), 2, 2)
    m8 = latte_amd.Latte(**small).to("cuda")
    assert lib.latte_trainer_create_joint(m8.engine_config("f16"), 2, 2, h) != 0
    with pytest.raises(latte_amd.LatteError):                                            # the model class is still refused by name
        latte_amd.get_models(types.SimpleNamespace(model="LatteIMG-S/2", latent_size=16, num_classes=5, num_frames=4, learn_sigma=True,
                                                   extras=2))


# ------------------------------------------------------------------------------------------------ 5. / 6. other kernels' shapes
def test_resident_attention_backward_at_the_image_pass_sequence_count():
    """T = 256 tokens per frame: the spatial attention backward's resident kernel, with B N = 4 sequences in the image pass."""
    check_parity("T256::F2::N2", case(2, images=2, batch=2, depth=2, input_size=32, num_frames=2), 2)


def test_head_dim_72():
    check_parity("hd72::F2::N1", case(2, images=1, batch=1, depth=2, hidden_size=1152, num_heads=16, num_frames=2), 1)


# ------------------------------------------------------------------------------------------------ 7. accumulation
def test_two_joint_micro_batches_accumulate_to_the_whole_batch():
    mkw, cfg, sd, (x0, noise, t, y, yi, drop, idrop), *_ = case(2, batch=2)
    whole, _ = trainer(mkw, sd, 2, jr.J_IMAGES)
    whole.forward_backward(x0, t, noise, y, drop, y_image=yi, image_drop_mask=idrop)
    one = grads_of(whole)
    del whole
    got = {}
    for staged in (False, True):
        tr, _ = trainer(mkw, sd, 1, jr.J_IMAGES, gradient_accumulation_steps=2, start_clip_iter=0)
        tr.always_staged = staged
        tr.grads.fill_(7.0)                                    # micro-batch 1's video pass assigns: nothing stale survives
        for i in range(2):
            sl = slice(i, i + 1)
            if i == 0:
                out, last = tr.backward_micro_batch(x0[sl], t[sl], noise[sl], y[sl], drop[sl], yi[sl], idrop[sl])
                assert not last
            else:
                out, last = tr.backward_micro_batch(x0[sl], t[sl], noise[sl], y[sl], drop[sl], yi[sl], idrop[sl])
                assert last
        got[staged] = grads_of(tr)
        del tr
    # Against the engine's own whole-batch joint step the operand roundings are the same (every row is computed alike in a batch of 1
    # and of 2; the loss weights 1 / (2 * 7/4), 1 / (2 * 7/3) of the window are the whole batch's exactly, a factor 2 apart from the
    # single pass's); only the order of the fp32 sums over rows differs: the bound of tests/test_train_accum.py for that.
    order = {k: rel(got[False][k], one[k]) for k in one}
    print("accumulated against the whole-batch joint step: worst", max(order, key=order.get), max(order.values()))
    assert max(order.values()) < 2e-6, {k: v for k, v in order.items() if not v < 2e-6}
    for k in one:                                              # the staged (bucketed) backward: the same launches, the same bits
        assert torch.equal(got[False][k], got[True][k]), k
    # train_step: the optimiser step runs after the window's second micro-batch only
    tr, _ = trainer(mkw, sd, 1, jr.J_IMAGES, gradient_accumulation_steps=2)
    o1 = tr.train_step(x0[:1], y=y[:1], t=t[:1], noise=noise[:1], drop_mask=drop[:1], y_image=yi[:1], image_drop_mask=idrop[:1])
    assert o1["updated"] is False and "grad_norm" not in o1 and tr.train_steps == 0 and tr.micro_step == 1
    o2 = tr.train_step(x0[1:2], y=y[1:2], t=t[1:2], noise=noise[1:2], drop_mask=drop[1:2], y_image=yi[1:2], image_drop_mask=idrop[1:2])
    assert o2["updated"] is True and "grad_norm" in o2 and tr.train_steps == 1 and tr.micro_step == 0
    flat = torch.cat([one[k].reshape(-1) for k in sorted(one)]).double().norm()
    assert abs(float(o2["grad_norm"]) - float(flat)) < 1e-5 * float(flat)


# ------------------------------------------------------------------------------------------------ 8. a full train_step
def test_full_joint_train_step_against_the_oracle_optimiser():
    mkw, cfg, sd, (x0, noise, t, y, yi, drop, idrop), *_ = case(2)
    probe, _ = trainer(mkw, sd, 3, jr.J_IMAGES)
    probe.forward_backward(x0, t, noise, y, drop, y_image=yi, image_drop_mask=idrop)
    g = grads_of(probe)                                        # the engine's gradients (deterministic: the step below computes the same)
    del probe
    tr, model = trainer(mkw, sd, 3, jr.J_IMAGES, start_clip_iter=0)                      # clipping on from the first step
    out = tr.train_step(x0, y=y, t=t, noise=noise, drop_mask=drop, y_image=yi, image_drop_mask=idrop)
    torch.cuda.synchronize()
    assert out["updated"] is True
    total, clipped = to.clip_grads(g, 0.1, clip=True)
    assert abs(float(out["grad_norm"]) - float(total)) < 1e-5 * float(total)
    new_sd, _ = to.adamw_step(sd, clipped, {}, 1, lr=1e-4)
    ema = to.update_ema({k: sd[k] for k in new_sd}, new_sd, 0.9999)
    msd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    esd = {k: v.cpu() for k, v in tr.ema_state_dict().items()}
    for k in g:
        assert float((msd[k] - new_sd[k]).abs().max()) < 3e-7, k
        assert float((esd[k] - ema[k]).abs().max()) < 3e-7, k
    assert float(tr.grads.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ 9. the two helper kernels
@pytest.mark.parametrize("B,F,N,per", [(3, 4, 3, 1024), (2, 2, 2, 4096), (1, 16, 8, 4100), (5, 3, 1, 7), (2, 1, 1, 1)])
def test_joint_split_and_merge_kernels(B, F, N, per):
    from latte_amd._lib import check, load_library, ptr, stream_ptr
    lib = load_library()
    g = torch.Generator("cpu").manual_seed(B * 1000 + per)
    x = torch.randn(B, F + N, per, generator=g).cuda()
    nz = torch.randn(B, F + N, per, generator=g).cuda()
    t = torch.randint(0, 1000, (B,), generator=g).cuda()
    xv, nv = torch.full((B, F, per), -7.0).cuda(), torch.full((B, F, per), -7.0).cuda()
    xi, ni = torch.full((B * N, per), -7.0).cuda(), torch.full((B * N, per), -7.0).cuda()
    ti = torch.full((B * N,), -1, dtype=torch.int64).cuda()
    check(lib.latte_debug_joint_split(ptr(x), ptr(nz), ptr(t), ptr(xv), ptr(nv), ptr(xi), ptr(ni), ptr(ti), B, F, N, per, stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(xv, x[:, :F]) and torch.equal(nv, nz[:, :F])                      # copies: exact
    assert torch.equal(xi, x[:, F:].reshape(B * N, per)) and torch.equal(ni, nz[:, F:].reshape(B * N, per))
    assert torch.equal(ti, t.repeat_interleave(N))
    tv = (torch.rand(3, B, generator=g) * 3).cuda()
    tim = (torch.rand(3, B * N, generator=g) * 3).cuda()
    terms = torch.full((3, B), -7.0).cuda()
    joint = torch.full((B, F + N, per), -7.0).cuda()
    check(lib.latte_debug_joint_merge(ptr(tv), ptr(tim), ptr(terms), ptr(xv), ptr(xi), ptr(joint), B, F, N, per, stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(joint, x)                                                         # the scatter is the split's inverse
    want = (F * tv.double().cpu() + tim.double().cpu().reshape(3, B, N).sum(2)) / (F + N)
    # fp32 rounding of three operations (the product by F, the sum, the division), each at most half an ulp of a value <= the result's
    # magnitude bound sum |.| / (F + N): 3 * 2^-24 relative to that bound
    mag = (F * tv.double().cpu().abs() + tim.double().cpu().abs().reshape(3, B, N).sum(2)) / (F + N)
    assert bool(((terms.double().cpu() - want).abs() <= 3 * 2.0 ** -24 * mag).all())
    terms2 = torch.full((3, B), -7.0).cuda()
    check(lib.latte_debug_joint_merge(ptr(tv), ptr(tim), ptr(terms2), None, None, None, B, F, N, per, stream_ptr()))   # terms only
    torch.cuda.synchronize()
    assert torch.equal(terms2, terms)
    assert lib.latte_debug_joint_split(ptr(x), ptr(nz), ptr(t), ptr(xv), ptr(nv), ptr(xi), ptr(ni), ptr(ti), B, F, 0, per, stream_ptr()) != 0


# ------------------------------------------------------------------------------------------------ 10. the driver
def test_train_driver_runs_the_joint_config(tmp_path):
    """tools/train.py on configs/tiny_img_train.yaml (model: LatteIMG-S/2, use_image_num: 2, synthetic data): finite losses, and a
    checkpoint with the key set of the plain Latte-S/2 preset, which samples."""
    import subprocess
    import sys
    import latte_amd
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / "run")
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "train.py"), "--config", os.path.join(root, "configs", "tiny_img_train.yaml"),
                        "--out", out, "--max-steps", "4", "--log-every", "2"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Train Loss" in r.stdout and "Saved checkpoint" in r.stdout and "nan" not in r.stdout.lower(), r.stdout
    sd = latte_amd.find_model(os.path.join(out, "checkpoints", "0000004.pt"))
    m = latte_amd.Latte_models["Latte-S/2"](input_size=16, num_frames=4, num_classes=5, extras=2, max_batch=1)
    assert set(sd) == set(m.state_dict())
    m.load_state_dict(sd)
    m = m.to("cuda")
    z = torch.randn(1, 4, 4, 16, 16, device="cuda")
    x = latte_amd.create_diffusion("5").ddim_sample_loop(m.forward, z.shape, z, clip_denoised=False,
                                                         model_kwargs=dict(y=torch.tensor([2], device="cuda")), device="cuda")
    assert torch.isfinite(x).all()
