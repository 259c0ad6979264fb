"""Gradient accumulation on the training engine (LatteTrainer(gradient_accumulation_steps=A), engine options "grad_accumulate" /
"loss_divisor"): a batch of 4 run as two micro-batches of 2 against the fp32 oracle's gradient of ``loss.mean()`` on the whole
batch (the mean over 4 is half the sum of the two micro-batch means), at the tiny trainer configuration of
tests/test_training_step.py.  Its tensors cover both reductions of the weight-gradient partials: x_embedder.proj.weight
(128 x 16 = 2048 elements) and every bias take the scalar kernel, the block weights (>= 16384) the 16-byte one."""
import functools
import math

import pytest
import torch

from oracle import diffusion_oracle as do
from oracle import latte_oracle as lo
from oracle import train_oracle as to
from oracle.make_golden import TRAIN_STEP, train_step_inputs
from test_training_step import GTOL, rel      # the per-tensor relative-L2 bound of the training-step tests (f16 operands: 5e-4)

# Accumulation adds fp32 micro-batch gradients in fp32: no operand is rounded that the single-batch step does not round, so the
# bound of the single-batch gradients holds for the sum.
TOL = GTOL["f16"]
# The bf16 trainer runs without a loss scale: its second micro-batch takes the writers' add-without-unscale branch.  Same argument,
# bf16's bound of the single-batch step.
TOLS = {"f16": TOL, "bf16": GTOL["bf16"]}


@functools.lru_cache(maxsize=None)
def case(extras):
    """Weights, a batch of 4 and the oracle's whole-batch result, computed once.  Samples 0 - 2 are the training-step fixture's
    (t = 0, an interior step, the last one; sample 2's label dropped); sample 3 repeats sample 0's label in the OTHER micro-batch."""
    kw = dict(TRAIN_STEP, extras=extras)
    cfg = lo.LatteConfig(**kw)
    _, sd2, x3, n3, t3, y3, d3 = train_step_inputs()
    # GTOL is an empirical figure: the single-batch step's worst tensor ON THE FIXTURE'S WEIGHTS (blocks.1.adaLN_modulation.1.weight,
    # 3.8e-4) plus a margin.  It does not carry over to another draw of the weights: on lo.init_state_dict(cfg, seed=11) for the model
    # without the label table the plain single-batch step (batch 4, no accumulation) puts blocks.1.adaLN_modulation.1.{bias,weight} at
    # 5.36e-4 against this oracle, and the accumulated gradient equals that step's to 2e-7.  So the unconditional case keeps the
    # fixture's weights and leaves the table out (measured there: 3.5e-4, the same tensor, single-batch and accumulated alike).
    sd = sd2 if extras == 2 else {k: v for k, v in sd2.items() if not k.startswith("y_embedder.")}
    g = torch.Generator("cpu").manual_seed(43)
    x0 = torch.cat([x3, (torch.randn(1, *x3.shape[1:], generator=g) * 0.6).clamp(-1.0, 1.0)])
    noise = torch.cat([n3, torch.randn(1, *x3.shape[1:], generator=g)])
    t = torch.cat([t3, torch.tensor([250])])
    y = torch.cat([y3, y3[:1]]) if extras == 2 else None
    drop = torch.cat([d3, torch.tensor([False])]) if extras == 2 else None
    terms, _, grads = to.loss_and_grads(sd, cfg, do.Schedule(""), x0, t, noise, y, drop)
    return kw, cfg, sd, (x0, noise, t, y, drop), terms, grads


def micro(inputs, i, n=2):
    return tuple(None if v is None else v[i * n:(i + 1) * n] for v in inputs)


def trainer(extras, accum=None, fuse_small=1, dt="f16", **kw):
    import latte_amd
    mkw, _, sd, _, _, _ = case(extras)
    model = latte_amd.Latte(**mkw)
    model.load_state_dict(sd)
    if accum is not None:
        kw["gradient_accumulation_steps"] = accum
    kw.setdefault("start_clip_iter", 10 ** 9)
    tr = latte_amd.LatteTrainer(model.to("cuda"), latte_amd.create_diffusion(""), max_batch=2, compute_dtype=dt, **kw)
    if not fuse_small:
        tr.set_option("fuse_small", 0)
    return tr, model


@functools.lru_cache(maxsize=None)
def whole_batch(extras, fuse_small, dt="f16"):
    """The engine's own gradient of the batch of 4 in ONE assigning forward_backward (the path without accumulation), once per case."""
    import latte_amd
    kw, _, sd, (x0, noise, t, y, drop), _, _ = case(extras)
    model = latte_amd.Latte(**kw)
    model.load_state_dict(sd)
    tr = latte_amd.LatteTrainer(model.to("cuda"), latte_amd.create_diffusion(""), max_batch=4, compute_dtype=dt, start_clip_iter=10 ** 9)
    tr.set_option("fuse_small", fuse_small)
    tr.forward_backward(x0, t, noise, y, drop)
    torch.cuda.synchronize()
    return {k: v.cpu().clone() for k, v in tr.grad_dict().items()}


def window(tr, inputs):
    """Both micro-batches of the window, no optimiser step -> the reported terms of each."""
    outs = []
    for i in range(2):
        x0, noise, t, y, drop = micro(inputs, i)
        out, last = tr.backward_micro_batch(x0, t, noise, y, drop)
        assert last == (i == 1)
        outs.append(out)
    torch.cuda.synchronize()
    return outs


def check_against_oracle(tr, grads_ref, label, tol=TOL):
    got = {k: v.cpu() for k, v in tr.grad_dict().items()}
    assert set(got) == set(grads_ref)
    worst = {k: rel(got[k], grads_ref[k]) for k in grads_ref}
    print(label, "worst gradient tensor", max(worst, key=worst.get), max(worst.values()))
    for k in ("blocks.0.attn.qkv.bias", "blocks.1.mlp.fc2.bias", "blocks.0.adaLN_modulation.1.bias", "final_layer.linear.weight",
              "final_layer.linear.bias", "final_layer.adaLN_modulation.1.weight", "x_embedder.proj.weight", "x_embedder.proj.bias",
              "t_embedder.mlp.0.weight", "t_embedder.mlp.2.bias"):
        assert k in worst, k                  # the writers most easily left in assign mode are among the compared tensors
        print("   ", k, worst[k])
    bad = {k: round(v, 6) for k, v in worst.items() if not v < tol}
    assert not bad, bad
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("extras,fuse_small,dt", [(e, f, dt) for dt in ("f16", "bf16") for e, f in ((2, 1), (2, 0), (1, 1), (1, 0))],
                         ids=[f"{e}-{f}" + ("" if dt == "f16" else "-bf16") for dt in ("f16", "bf16") for e, f in ((2, 1), (2, 0), (1, 1), (1, 0))])
def test_accumulated_gradients_match_the_oracle_on_the_whole_batch(extras, fuse_small, dt):
    _, _, _, inputs, terms, grads_ref = case(extras)
    sizes = sorted(g.numel() for g in grads_ref.values())
    assert sizes[0] < 4096 <= sizes[-1]                      # both reductions of the partial products write gradients here
    tr, _ = trainer(extras, accum=2, fuse_small=fuse_small, dt=dt)
    assert (tr.scaler_state()["loss_scale"] > 1.0) == (dt == "f16")   # bf16: no loss scale, the writers add without unscaling
    outs = window(tr, inputs)
    got = check_against_oracle(tr, grads_ref, f"extras {extras} fuse_small {fuse_small} {dt}", TOLS[dt])
    # Against the engine's own whole-batch step the operand roundings are the same (every row is computed alike in a batch of 2 and
    # of 4, the loss weight 2 / (per * 2 * 2) is the whole batch's exactly); only the order of fp32 sums over the 256 rows differs:
    # sqrt(256) * 2^-24 = 1e-6 of the summed magnitudes, which exceed the result's norm by up to 1.6 x here -> 2e-6.
    one = whole_batch(extras, fuse_small, dt)
    order = {k: rel(got[k], one[k]) for k in one}
    print("    against the single whole-batch step: worst", max(order, key=order.get), max(order.values()))
    assert max(order.values()) < 2e-6, {k: v for k, v in order.items() if not v < 2e-6}
    if extras == 2:                                        # rows of the label table: class 1 (both micro-batches), the null class (dropped)
        gy = tr.grad_dict()["y_embedder.embedding_table.weight"].cpu()
        for row in (1, 4, 5):                              # (their values: the tensor's bound above; a cleared or doubled row breaks it)
            assert float(gy[row].abs().max()) > 0.0, row
        for row in (0, 2, 3):                              # labels no sample carries (2 was dropped): never written
            assert float(gy[row].abs().max()) == 0.0, row
    for i, out in enumerate(outs):                          # the reported terms are NOT divided by the window length
        for k in ("loss", "mse", "vb"):
            assert rel(out[k].cpu(), terms[k][2 * i:2 * i + 2]) < 1e-4, (i, k)


@pytest.mark.gpu
@pytest.mark.parametrize("fuse_small,dt", [(1, "f16"), (0, "f16"), (1, "bf16"), (0, "bf16")], ids=["1", "0", "1-bf16", "0-bf16"])
def test_first_micro_batch_assigns_over_a_stale_buffer(fuse_small, dt):
    """Micro-batch 1 of a window runs in assign mode: whatever the gradient buffer held does not leak into the window."""
    _, _, _, inputs, _, grads_ref = case(2)
    clean, _ = trainer(2, accum=2, fuse_small=fuse_small, dt=dt)
    window(clean, inputs)
    dirty, _ = trainer(2, accum=2, fuse_small=fuse_small, dt=dt)
    for k, off, numel in dirty.layout:
        dirty.grads[off:off + numel].fill_(1.0e6)
    window(dirty, inputs)
    check_against_oracle(dirty, grads_ref, f"stale buffer, fuse_small {fuse_small} {dt}", TOLS[dt])
    for k, off, numel in dirty.layout:
        assert torch.equal(dirty.grads[off:off + numel], clean.grads[off:off + numel]), k


@pytest.mark.gpu
def test_defaults_are_unchanged():
    """gradient_accumulation_steps=1 is the trainer without the argument: the same bits after two steps."""
    _, _, _, inputs, _, _ = case(2)
    res = []
    for accum in (None, 1):
        tr, _ = trainer(2, accum=accum)
        for i in range(2):
            x0, noise, t, y, drop = micro(inputs, i)
            out = tr.train_step(x0, y=y, t=t, noise=noise, drop_mask=drop)
            assert out["updated"] and "grad_norm" in out
        torch.cuda.synchronize()
        res.append([b.clone() for b in (tr.params, tr.ema, tr.exp_avg, tr.exp_avg_sq)])
    for a, b in zip(*res):
        assert torch.equal(a, b)


@pytest.mark.gpu
def test_one_update_per_window():
    _, _, _, inputs, terms, _ = case(2)
    tr, _ = trainer(2, accum=2)
    p0 = tr.params.clone()
    for n in range(4):
        x0, noise, t, y, drop = micro(inputs, n % 2)
        out = tr.train_step(x0, y=y, t=t, noise=noise, drop_mask=drop)
        assert out["updated"] == (n % 2 == 1)
        assert ("grad_norm" in out) == (n % 2 == 1)
        assert tr.scaler_state()["applied_updates"] == float((n + 1) // 2)
        assert tr.train_steps == (n + 1) // 2 and tr.micro_step == (n + 1) % 2
        if n == 0:
            assert torch.equal(tr.params, p0)                # nothing moves inside a window
        if n < 2:                                            # (the parameters of the first window are the oracle's)
            for k in ("loss", "mse", "vb"):
                assert rel(out[k].cpu(), terms[k][2 * n:2 * n + 2]) < 1e-4, (n, k)
    assert not torch.equal(tr.params, p0)
    assert float(tr.grads.abs().max()) == 0.0                # the step leaves the gradient buffer zeroed


@pytest.mark.gpu
def test_accumulated_update_matches_the_oracle():
    """After one accumulated window: clip + AdamW + EMA.  As in test_engine_train_step_vs_reference_fixture the oracle's update
    rule runs on the gradients the engine accumulated (AdamW's first step is -lr sign(g): on the oracle's own gradients every
    element whose sign the operand rounding flips would differ by 2 lr), which the oracle comparison above ties to the
    whole-batch gradient; the tolerance is that test's 3e-7.  Clipping is on from the first step here, at half the gradient's norm."""
    _, _, sd, inputs, _, grads_ref = case(2)
    max_norm = 0.5 * float(to.grad_norm(grads_ref))          # half the whole-batch norm: the coefficient is about 0.5, not 1
    tr, model = trainer(2, accum=2, start_clip_iter=0, clip_max_norm=max_norm)
    window(tr, inputs)
    got = check_against_oracle(tr, grads_ref, "update")
    total, clipped = to.clip_grads(got, max_norm, clip=True)
    gn = tr.optimizer_step()
    torch.cuda.synchronize()
    assert abs(float(gn) - float(total)) < 1e-5 * float(total)
    new_sd, _ = to.adamw_step(sd, clipped, {}, 1, lr=1e-4)
    ema = to.update_ema({k: sd[k] for k in new_sd}, new_sd, 0.9999)
    msd = {k: v.cpu() for k, v in tr.model_state_dict().items()}
    esd = {k: v.cpu() for k, v in tr.ema_state_dict().items()}
    for k in got:
        assert float((msd[k] - new_sd[k]).abs().max()) < 3e-7, k
        assert float((esd[k] - ema[k]).abs().max()) < 3e-7, k
    assert tr.micro_step == 0 and tr.train_steps == 1


# ------------------------------------------------------------------------------------------------ the optimiser's trajectory
TRAJ = dict(lr=1e-4, b1=0.9, b2=0.999, eps=1e-8, wd=0.05, decay=0.9999)
TRAJ_SCALES = (1.0, 0.7, 1.5, 1.2, 0.45, 2.0)       # gradient norm of each step in units of 2 x clip_max_norm: the fifth is not clipped
TRAJ_INF_STEP = 2                                   # the third step's gradient holds one inf


def follow_adamw(tr, seed=7):
    """Six optimiser steps of `tr` (params / grads / exp_avg / exp_avg_sq / ema flat fp32 buffers, clip_max_norm, optimizer_step(),
    scaler_state()) on injected gradients against torch.optim.AdamW + clip_grad_norm_ + update_ema on float64 CPU copies; see
    test_six_optimiser_steps_follow_torch_adamw.  -> worst err / bound per buffer."""
    import numpy as np
    from test_optimizer_kernels import U32, adamw_ref, scaler_model
    f32 = lambda x: float(np.float32(x))
    h = {k: f32(v) for k, v in TRAJ.items()}
    n = tr.params.numel()
    gen = torch.Generator("cpu").manual_seed(seed)
    base = 1e-3
    tr.clip_max_norm = f32(0.5 * base * n ** 0.5)
    p64 = torch.nn.Parameter(tr.params.detach().double().cpu().clone())
    ema64 = tr.ema.detach().double().cpu().clone()
    opt = torch.optim.AdamW([p64], lr=h["lr"], betas=(h["b1"], h["b2"]), eps=h["eps"], weight_decay=h["wd"])
    zero = torch.zeros(n, dtype=torch.float64)
    E = dict(p=zero.clone(), m=zero.clone(), v=zero.clone(), ema=zero.clone())
    sc = list(tr.scaler_state().values())
    applied, worst = 0, {}
    for i, s in enumerate(TRAJ_SCALES):
        g32 = torch.randn(n, generator=gen) * (base * s)
        if i == TRAJ_INF_STEP:
            g32[n // 3] = float("inf")
        tr.grads.copy_(g32)
        p64.grad = g32.double()
        norm = float(torch.nn.utils.clip_grad_norm_([p64], tr.clip_max_norm))
        ok = math.isfinite(norm)
        if ok:
            st = opt.state.get(p64, {})
            m0, v0 = st.get("exp_avg", zero).clone(), st.get("exp_avg_sq", zero).clone()
            p0, e0, gc = p64.detach().clone(), ema64.clone(), p64.grad.clone()
            opt.step()
            ema64.mul_(h["decay"]).add_(p64.detach(), alpha=1 - h["decay"])
            applied += 1
            # the step's own bounds at the reference state, then what the errors carried into it become (docstring)
            _, L = adamw_ref(p0, gc, m0, v0, e0, h, applied, 1.0)
            m1, v1 = opt.state[p64]["exp_avg"], opt.state[p64]["exp_avg_sq"]
            bc1, bc2 = 1 - h["b1"] ** applied, 1 - h["b2"] ** applied
            denom = v1.sqrt() / math.sqrt(bc2) + h["eps"]
            upd = h["lr"] / bc1 * m1 / denom
            cm = 4 * U32 * (1 - h["b1"]) * gc.abs()                # the clip coefficient's 4 roundings, through g'
            cv = 8 * U32 * (1 - h["b2"]) * gc * gc
            in_m, in_v = h["b1"] * E["m"] + cm, h["b2"] * E["v"] + cv
            Ep = (1 - h["lr"] * h["wd"]) * E["p"] + L["p"] + h["lr"] / bc1 * in_m / denom + upd.abs() * in_v / (2 * v1)
            E = dict(m=in_m + L["m"], v=in_v + L["v"], p=Ep, ema=h["decay"] * E["ema"] + L["ema"] + (1 - h["decay"]) * (Ep - L["p"]))
        p64.grad = None
        before = [t.clone() for t in (tr.params, tr.ema, tr.exp_avg, tr.exp_avg_sq)]
        gn = tr.optimizer_step()
        if not ok:
            assert all(torch.equal(a, b) for a, b in zip(before, (tr.params, tr.ema, tr.exp_avg, tr.exp_avg_sq))), "the skipped step moved a buffer"
        sc = scaler_model(sc, ok)
        assert list(tr.scaler_state().values()) == sc, f"step {i + 1}: counters {tr.scaler_state()} against {sc}"
        assert math.isfinite(float(gn)) == ok and float(tr.grads.abs().max()) == 0.0
        if ok:
            assert abs(float(gn) - norm) <= 2 * U32 * norm
        st = opt.state.get(p64, {})
        for k, got, want in (("p", tr.params, p64.detach()), ("ema", tr.ema, ema64), ("m", tr.exp_avg, st.get("exp_avg", zero)),
                             ("v", tr.exp_avg_sq, st.get("exp_avg_sq", zero))):
            err = (got.detach().double().cpu() - want).abs()
            bad = ~(err <= E[k])
            assert not bool(bad.any()), (f"step {i + 1} ({applied} applied): {k}: {int(bad.sum())} of {n} elements out of bound, worst err / bound "
                                         f"{float((err / E[k].clamp_min(1e-300)).max()):.3g}")
            if ok:
                worst[k] = max(worst.get(k, 0.0), float((err / E[k]).max()))
    assert applied == len(TRAJ_SCALES) - 1 and sc[2] == applied and sc[3] == 1.0
    return worst


@pytest.mark.gpu
def test_six_optimiser_steps_follow_torch_adamw():
    """weight_decay 0.05, clipping from the first step at half the norm of the first gradient; six steps on gradients written straight
    into tr.grads (seeded, another draw and another norm per step -- the fifth stays below the clip norm), the third with one inf.  The
    reference is torch.optim.AdamW ITSELF on a float64 CPU copy of the flat parameter buffer, fed by clip_grad_norm_, followed by
    update_ema; its step() is not called at the skipped step, so its bias corrections count 5 -- an engine that counted the skipped
    call would sit at 6 and miss the parameters by about 1 / 6 of a step's update from the fourth step on.  After EVERY step: params,
    ema, exp_avg, exp_avg_sq within the accumulated bound, the eight scaler counters equal to the state machine's model.

    Accumulation (first order).  L_x is the one-step bound of test_optimizer_kernels.adamw_ref at the reference's state, E_x the bound
    carried into the step.  The engine's clip coefficient passes 4 fp32 roundings the reference does not (the norm to fp32, + 1e-6
    and the constant itself, the divide): c_m = 4 u (1 - b1) |g'| on m', c_v = 8 u (1 - b2) g'^2 on v'.  Then
        E_m' = b1 E_m + c_m + L_m                      E_v' = b2 E_v + c_v + L_v
        E_p' = (1 - lr wd) E_p + L_p + (lr / bc1) (b1 E_m + c_m) / denom + |upd| (b2 E_v + c_v) / (2 v')
        E_ema' = d E_ema + L_ema + (1 - d) (E_p' - L_p)
    (d upd / d m' = (lr / bc1) / denom; |d upd / d v'| <= |upd| / (2 v'); L_ema already holds (1 - d) L_p).  A skipped step carries every
    E over unchanged, and the buffers must not move at all."""
    tr, model = trainer(2, weight_decay=TRAJ["wd"], start_clip_iter=0, lr=TRAJ["lr"], ema_decay=TRAJ["decay"])
    worst = follow_adamw(tr)
    print("optimiser trajectory: worst err / accumulated bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
