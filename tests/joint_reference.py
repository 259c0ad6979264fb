"""fp32 restatement of joint image-video training: ``LatteIMG.forward`` in train mode (models/latte_img.py:316-399) plus
``training_losses`` (gaussian_diffusion.py:719-795) -> terms, model output and the gradients of ``terms['loss'].mean()``.

Built on the pinned CPU oracles (``oracle.latte_oracle._block``, ``oracle.diffusion_oracle.q_sample`` / ``_vb_terms_bpd``).
tests/test_joint_reference.py pins it to the committed fixture tests/golden/train_joint.npz -- what the reference objects
computed (tools/make_joint_golden.py) -- and, where the reference is present, to the live reference.

What LatteIMG does with a sample of F video frames and N image frames (``use_image_num`` = N):
  * every spatial block runs on all F + N frames, frame by frame; frame f < F is conditioned on t + emb(y), image n on
    t + emb(y_image[n]) (:334-346,:365); the final layer uses the same per-frame conditioning (:391-395);
  * the temporal blocks see x[:, :F] only, conditioned on t + emb(y); temp_embed is added to those F frames in front of block 1
    (:372-389);
  * label dropout happens BEFORE this function (one coin per sample for y, one per sample for all of its images, :341-342 with
    ``token_drop``'s rand(labels.shape[0])): dropped labels arrive as ``num_classes``.

``image_pass`` is the same network on B N one-frame samples with the temporal blocks off -- the second half of the decomposition
  terms_b = (F terms_video_b + sum_n terms_image_{b,n}) / (F + N)
  grad loss.mean() = F / (F + N) grad mean_b(loss_video_b) + N / (F + N) grad mean_{b,n}(loss_image_{b,n})
that the engine's joint step runs (include/latte_amd.h); the video half is ``oracle.train_oracle.loss_and_grads``."""
import importlib.util
import os
import sys

import torch
import torch.nn.functional as F

from oracle import diffusion_oracle as do
from oracle import latte_oracle as lo
from oracle import reference_loader as rl
from oracle.train_oracle import FROZEN, trainable_keys

# Fixture J (tests/golden/train_joint.npz): depth 4 puts a skipped temporal block between two spatial ones; T = 64 tokens per frame;
# the image pass has 3 * 3 * 64 = 576 rows -- no multiple of 128
J_MODEL = dict(depth=4, hidden_size=128, patch_size=2, num_heads=2, input_size=16, num_frames=4, num_classes=5, extras=2, learn_sigma=True)
J_IMAGES = 3
J_SEED = 17


def joint_inputs(model=None, images=J_IMAGES, batch=3, seed=23, weight_seed=J_SEED):
    """-> cfg, sd, x0 [B, F + N, C, H, W], noise, t, y, y_image [B, N], drop [B], image_drop [B].  Defaults: fixture J -- t = 0 (decoder
    NLL), an interior step, the last one; sample 2's video label and sample 1's image labels dropped; sample 0 repeats a label inside
    the sample, sample 2's first image carries sample 1's video label."""
    cfg = lo.LatteConfig(**(model or J_MODEL))
    sd = lo.init_state_dict(cfg, seed=weight_seed)
    g = torch.Generator("cpu").manual_seed(seed)
    shape = (batch, cfg.num_frames + images, cfg.in_channels, cfg.input_size, cfg.input_size)
    x0 = (torch.randn(*shape, generator=g) * 0.6).clamp(-1.0, 1.0)
    noise = torch.randn(*shape, generator=g)
    t = torch.tensor([0, 500, 999, 250, 750, 1][:batch], dtype=torch.int64)
    y = torch.tensor([1, 4, 2, 0, 3, 1][:batch], dtype=torch.int64)
    y_image = torch.tensor([[3, 3, 0], [2, 1, 0], [4, 0, 1], [1, 2, 3], [0, 0, 4], [2, 4, 1]], dtype=torch.int64)
    y_image = y_image.repeat(1, (images + 2) // 3)[:batch, :images].contiguous()
    drop = torch.tensor([False, False, True, False, False, False][:batch])
    image_drop = torch.tensor([False, True, False, False, False, True][:batch])
    if cfg.extras != 2:
        y = y_image = drop = image_drop = None
    return cfg, sd, x0, noise, t, y, y_image, drop, image_drop


def dropped(labels, mask, num_classes):
    """LabelEmbedder.token_drop with the coin given (latte.py:146-148); mask [B] broadcasts over a sample's images."""
    if labels is None or mask is None:
        return labels
    m = mask.reshape(-1, *([1] * (labels.dim() - 1)))
    return torch.where(m, torch.full_like(labels, num_classes), labels)


def _embed(sd, cfg, x, t_orig):
    B, Fr, C, H, W = x.shape
    tok = F.conv2d(x.reshape(B * Fr, C, H, W).float(), sd["x_embedder.proj.weight"], sd["x_embedder.proj.bias"], stride=cfg.patch_size)
    tok = tok.flatten(2).transpose(1, 2) + sd["pos_embed"]
    temb = lo.timestep_embedding(t_orig, 256)
    temb = F.linear(temb, sd["t_embedder.mlp.0.weight"], sd["t_embedder.mlp.0.bias"])
    temb = F.linear(F.silu(temb), sd["t_embedder.mlp.2.weight"], sd["t_embedder.mlp.2.bias"])
    return tok, temb


def _final(sd, cfg, h, c_frames, B, Fr, H):
    D, p, co = cfg.hidden_size, cfg.patch_size, cfg.out_channels
    mod = F.linear(F.silu(c_frames), sd["final_layer.adaLN_modulation.1.weight"], sd["final_layer.adaLN_modulation.1.bias"])
    shift, scale = mod.chunk(2, dim=1)
    h = lo._modulate(F.layer_norm(h, (D,), eps=1e-6), shift, scale)
    h = F.linear(h, sd["final_layer.linear.weight"], sd["final_layer.linear.bias"])
    gh = H // p
    h = h.reshape(B * Fr, gh, gh, p, p, co).permute(0, 5, 1, 3, 2, 4).reshape(B * Fr, co, gh * p, gh * p)
    return h.reshape(B, Fr, co, H, H)


def joint_forward(sd, cfg, x, t_orig, y, y_image, images):
    """LatteIMG.forward, train mode; x [B, F + N, C, H, W], labels after dropout -> [B, F + N, C_out, H, W]."""
    B, FN, C, H, W = x.shape
    Fr, D = FN - images, cfg.hidden_size
    assert Fr == cfg.num_frames
    tok, temb = _embed(sd, cfg, x, t_orig)
    T = tok.shape[1]
    if cfg.extras == 2:
        table = sd["y_embedder.embedding_table.weight"]
        yv = table[y]                                                                       # [B, D]
        y_frames = torch.cat([yv[:, None].expand(B, Fr, D), table[y_image]], dim=1)          # :344-346
        c_frames = (temb[:, None] + y_frames).reshape(B * FN, D)
        c_temp = (temb + yv).repeat_interleave(T, dim=0)
    else:
        c_frames = temb.repeat_interleave(FN, dim=0)
        c_temp = temb.repeat_interleave(T, dim=0)
    h = tok
    for i in range(0, cfg.depth, 2):
        h = lo._block(sd, i, h, c_frames, cfg.num_heads).reshape(B, FN, T, D)
        hv = h[:, :Fr].permute(0, 2, 1, 3).reshape(B * T, Fr, D)                              # :372-373
        if i == 0:
            hv = hv + sd["temp_embed"]
        hv = lo._block(sd, i + 1, hv, c_temp, cfg.num_heads)
        hv = hv.reshape(B, T, Fr, D).permute(0, 2, 1, 3)
        h = torch.cat([hv, h[:, Fr:]], dim=1).reshape(B * FN, T, D)                           # :388-389
    return _final(sd, cfg, h, c_frames, B, FN, H)


def image_forward(sd, cfg, x, t_orig, y):
    """The spatial-only network on one-frame samples: x [S, 1, C, H, W], t_orig [S], y [S] | None -> [S, 1, C_out, H, W]."""
    S, one, C, H, W = x.shape
    assert one == 1
    tok, temb = _embed(sd, cfg, x, t_orig)
    c = temb + sd["y_embedder.embedding_table.weight"][y] if cfg.extras == 2 else temb
    h = tok
    for i in range(0, cfg.depth, 2):
        h = lo._block(sd, i, h, c, cfg.num_heads)
    return _final(sd, cfg, h, c, S, 1, H)


def _terms(sched, out, x_start, x_t, noise, t, loss_type):
    C = x_t.shape[2]
    terms = {}
    if sched.var_type == "learned_range":
        eps, v = out[:, :, :C], out[:, :, C:]
        terms["vb"] = do._vb_terms_bpd(sched, torch.cat([eps.detach(), v], dim=2), x_start, x_t, t)   # gd:753-757
        if loss_type == "rescaled_mse":
            terms["vb"] = terms["vb"] * (sched.num_timesteps / 1000.0)
    else:
        eps = out
    terms["mse"] = do._mean_flat(((x_start if sched.predict_xstart else noise) - eps) ** 2)
    terms["loss"] = terms["mse"] + terms["vb"] if "vb" in terms else terms["mse"]
    return terms


def _run(sd, sched, model_fn, x_start, t, noise, loss_type):
    params = {k: (v.detach().clone().requires_grad_(k not in FROZEN)) for k, v in sd.items()}
    x_t = do.q_sample(sched, x_start, t, noise)
    t_orig = torch.tensor(sched.timestep_map, dtype=torch.int64)[t]
    out = model_fn(params, x_t, t_orig)
    terms = _terms(sched, out, x_start, x_t, noise, t, loss_type)
    keys = trainable_keys(params)
    grads = torch.autograd.grad(terms["loss"].mean(), [params[k] for k in keys], allow_unused=True)
    grads = {k: (torch.zeros_like(params[k]) if g is None else g) for k, g in zip(keys, grads)}
    return {k: v.detach() for k, v in terms.items()}, out.detach(), grads


def joint_loss_and_grads(sd, cfg, sched, x_start, t, noise, y=None, y_image=None, drop_mask=None, image_drop_mask=None, images=J_IMAGES,
                         loss_type="mse"):
    """train_with_img.py:214-241 for one micro-batch -> (terms {k: [B]}, model output, {key: gradient of terms['loss'].mean()})."""
    yy, yi = dropped(y, drop_mask, cfg.num_classes), dropped(y_image, image_drop_mask, cfg.num_classes)
    return _run(sd, sched, lambda p, x_t, t_orig: joint_forward(p, cfg, x_t, t_orig, yy, yi, images), x_start, t, noise, loss_type)


def image_pass(sd, cfg, sched, x_images, t, noise_images, y_image=None, image_drop_mask=None, loss_type="mse"):
    """The image half of the decomposition: x_images / noise_images [B, N, C, H, W] as B N one-frame samples with t_b and their own
    labels -> (terms {k: [B N]}, model output [B N, 1, ...], gradients of mean_{b,n}(loss); the temporal blocks' are zero)."""
    B, N = x_images.shape[:2]
    yi = dropped(y_image, image_drop_mask, cfg.num_classes)
    yi = None if yi is None else yi.reshape(B * N)
    tt = t.repeat_interleave(N)
    return _run(sd, sched, lambda p, x_t, t_orig: image_forward(p, cfg, x_t, t_orig, yi), x_images.reshape(B * N, 1, *x_images.shape[2:]),
                tt, noise_images.reshape(B * N, 1, *noise_images.shape[2:]), loss_type)


def loss_weights(frames, images):
    """(video, image) weights of the two passes' losses in the joint loss: F / (F + N), N / (F + N)."""
    return frames / (frames + images), images / (frames + images)


# ---- the committed fixture: small tensors whole, large ones as their norm and a fixed sample of elements (file size)
GOLD_SAMPLE = 4096


def sample_index(numel):
    """Every element of a tensor up to GOLD_SAMPLE elements, else GOLD_SAMPLE elements at a stride coprime to the usual row lengths."""
    if numel <= GOLD_SAMPLE:
        return torch.arange(numel)
    return (torch.arange(GOLD_SAMPLE, dtype=torch.int64) * 7919) % numel


# ---- the live reference (present where the fixture is generated; tools/make_joint_golden.py and the CPU test call this)
def load_reference_latte_img():
    assert rl.reference_available(), "reference checkout not present"
    rl._install_timm_standin()
    name = "_reference_latte_img"
    if name not in sys.modules:
        spec = importlib.util.spec_from_file_location(name, os.path.join(rl.REFERENCE_ROOT, "models", "latte_img.py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
    return sys.modules[name]


def reference_step(model_kw, sd, x0, noise, t, y, y_image, drop, image_drop, images):
    """-> (terms, model output, {key: gradient}) of the reference objects on the given weights and inputs."""
    ri, rd = load_reference_latte_img(), rl.load_reference_diffusion()
    model = ri.Latte(**model_kw)
    if model_kw.get("extras", 1) == 2:
        model.y_embedder.dropout_prob = 0.0
    model.load_state_dict(sd)
    model.train()
    nc = model_kw.get("num_classes", 1000)
    yy, yi = dropped(y, drop, nc), dropped(y_image, image_drop, nc)
    kwargs = dict(y=yy, use_image_num=images)
    if yi is not None:
        kwargs["y_image"] = [row for row in yi]          # train_with_img.py:218-221: a list of B tensors of N labels
    seen = {}
    hook = model.final_layer.register_forward_hook(lambda m, i, o: seen.__setitem__("tok", o.detach()))
    terms = rd.create_diffusion("").training_losses(model, x0, t, kwargs, noise=noise)
    hook.remove()
    terms["loss"].mean().backward()
    out = model.unpatchify(seen["tok"]).reshape(x0.shape[0], x0.shape[1], -1, x0.shape[3], x0.shape[4])
    grads = {k: (p.grad.clone() if p.grad is not None else torch.zeros_like(p)) for k, p in model.named_parameters() if p.requires_grad}
    return {k: v.detach() for k, v in terms.items()}, out, grads
