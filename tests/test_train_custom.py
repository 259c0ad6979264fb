"""Custom losses on the training engine: ``LatteTrainer.forward`` (latte_trainer_forward) returns the model output as a node of the
torch autograd graph, whose backward seeds the engine's staged backward (latte_trainer_seed) and returns the gradient of the model
INPUT (latte_trainer_input_grad) -- at the training-step fixture (oracle.make_golden.TRAIN_STEP: depth 2, hidden 128, 2 heads,
16 tokens x 4 frames, 3 samples, learned sigma, one dropped label).  The yardstick is oracle.latte_oracle.latte_forward under torch
autograd on the CPU, as oracle/train_oracle.py uses it, on the x_t the engine's q_sample kernel made.

Bounds.  GTOL (tests/test_training_step.py) is the per-tensor relative L2 of the built-in loss's gradients on these weights
(measured worst tensor + 20 %).  The custom loss below goes through the same forward and the same backward kernels; only the seed
differs, so GTOL is the bound here too, for the parameters and for x.grad alike (x.grad comes from the same token gradient as
x_embedder.proj.weight's, through one fp32 kernel).  The measured worst tensors go into the JSON file LATTE_CUSTOM_PARITY_JSON names
(profiles/train_custom_parity.json was written so): the custom loss f16 4.13e-4 / bf16 3.43e-3 (blocks.1.adaLN_modulation.1.weight, the
built-in loss's worst tensor too), x.grad 2.1e-4 / 1.6e-3, train_step(loss_fn=mse) 3.9e-4 / 3.0e-3 -- all inside GTOL as it stands."""
import functools
import json
import os

import pytest
import torch
import torch.nn.functional as F

from oracle import diffusion_oracle as do
from oracle import latte_oracle as lo
from oracle import train_oracle as to
from oracle.make_golden import TRAIN_STEP, train_step_inputs
from test_training_step import GTOL, rel

pytestmark = pytest.mark.gpu

DTYPES = ["f16", "bf16"]
WEIGHTS = (0.3, 1.0, 2.5)        # per-sample loss weights of the custom loss
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def custom_per_sample(out, noise, w):
    """w_b mean((noise - eps)^2) + 0.05 mean(smooth_l1(v)) per sample: a weighted MSE on the mean head, a Huber regulariser on the
    variance head.  Its mean over the batch is L = mean_b[w_b mse_b] + 0.05 mean(smooth_l1(v))."""
    C = noise.shape[2]
    eps, v = out[:, :, :C], out[:, :, C:]
    mse = ((noise - eps) ** 2).flatten(1).mean(1)
    reg = F.smooth_l1_loss(v, torch.zeros_like(v), reduction="none").flatten(1).mean(1)
    return w * mse + 0.05 * reg


def weighted_loss_fn(out, x_start, x_t, t, noise):
    return custom_per_sample(out, noise, torch.tensor(WEIGHTS[:out.shape[0]], device=out.device))


def mse_loss_fn(out, x_start, x_t, t, noise):
    return ((noise - out) ** 2).flatten(1).mean(1)


@functools.lru_cache(maxsize=None)
def inputs():
    cfg, sd, x0, noise, t, y, drop = train_step_inputs()
    yd = torch.where(drop, torch.full_like(y, cfg.num_classes), y)          # the labels after dropout (latte.py:146-148)
    return cfg, sd, x0, noise, t, y, drop, yd


def trainer(dtype, accum=1, max_batch=3, kw_model=None, sd=None, diffusion=None, **kw):
    import latte_amd
    model = latte_amd.Latte(**(kw_model or TRAIN_STEP))
    model.load_state_dict(sd if sd is not None else inputs()[1])
    kw.setdefault("start_clip_iter", 10 ** 9)
    return latte_amd.LatteTrainer(model.to("cuda"), diffusion or latte_amd.create_diffusion(""), max_batch=max_batch, compute_dtype=dtype,
                                  gradient_accumulation_steps=accum, **kw)


@functools.lru_cache(maxsize=None)
def plain_diffusion():
    import latte_amd
    return latte_amd.create_diffusion("")


def engine_q_sample(x0, t, noise):
    """x_t by the engine's kernel (what the built-in step computes inside), on the GPU."""
    return plain_diffusion().q_sample(x0.cuda(), t.cuda(), noise.cuda())


def grads_of(tr):
    torch.cuda.synchronize()
    return {k: v.cpu().clone() for k, v in tr.grad_dict().items()}


def record(key, worst):
    """The measured worst tensor into the JSON file LATTE_CUSTOM_PARITY_JSON names; nothing is written without it."""
    path = os.environ.get("LATTE_CUSTOM_PARITY_JSON")
    if not path:
        return
    tab = json.load(open(path)) if os.path.exists(path) else {}
    tab[key] = {"worst_tensor": max(worst, key=worst.get), "worst_rel_l2": max(worst.values()),
                "median_rel_l2": sorted(worst.values())[len(worst) // 2]}
    json.dump(tab, open(path, "w"), indent=1, sort_keys=True)


@functools.lru_cache(maxsize=None)
def oracle_custom():
    """The oracle's gradients of the custom loss with respect to every trained parameter and to x_t, once."""
    cfg, sd, x0, noise, t, y, drop, yd = inputs()
    x_t = engine_q_sample(x0, t, noise).cpu().requires_grad_(True)
    params = {k: v.detach().clone().requires_grad_(k not in to.FROZEN) for k, v in sd.items()}
    out = lo.latte_forward(params, cfg, x_t, t, yd)                           # create_diffusion(""): timestep_map is the identity
    loss = custom_per_sample(out, noise, torch.tensor(WEIGHTS)).mean()
    keys = to.trainable_keys(params)
    g = torch.autograd.grad(loss, [params[k] for k in keys] + [x_t])
    return dict(zip(keys, g[:-1])), g[-1], float(loss.detach())


@functools.lru_cache(maxsize=None)
def engine_custom(dtype, staged=False):
    """One custom step on the fixture with x_t.requires_grad: (parameter gradients, x_t.grad, loss), once per operand type."""
    cfg, sd, x0, noise, t, y, drop, yd = inputs()
    tr = trainer(dtype)
    tr.always_staged = staged
    x_t = engine_q_sample(x0, t, noise).requires_grad_(True)
    out = tr.forward(x_t, t, y, drop_mask=drop)
    loss = custom_per_sample(out, noise.cuda(), torch.tensor(WEIGHTS, device="cuda")).mean()
    loss.backward()
    assert tr.micro_step == 1
    return grads_of(tr), x_t.grad.cpu().clone(), float(loss.detach())


# ------------------------------------------------------------------------------------------------ 1. the seam changes nothing
@pytest.mark.parametrize("accum", [1, 2])
@pytest.mark.parametrize("dtype", DTYPES)
def test_seam_is_bit_identical_to_the_builtin_step(dtype, accum):
    """forward + the built-in loss's own seed (latte_debug_loss_grad on the returned output) + backward = forward_backward, bit for bit:
    the same launches behind another entry point.  gradient_accumulation_steps = 2: the two-micro-batch window (2 + 1 samples); the
    seed is divided by the window length, a power of two, exactly -- as the built-in loss weight is."""
    from latte_amd._lib import check, load_library, ptr, stream_ptr
    cfg, sd, x0, noise, t, y, drop, yd = inputs()
    ref, cus = trainer(dtype, accum), trainer(dtype, accum)
    lib = load_library()
    Fr, C, H = cfg.num_frames, cfg.in_channels, cfg.input_size
    for i, (a, b) in enumerate([(0, 3)] if accum == 1 else [(0, 2), (2, 3)]):
        ref._set_accumulate(i > 0)                                             # what backward_micro_batch does
        r = ref.forward_backward(x0[a:b], t[a:b], noise[a:b], y[a:b], drop[a:b], return_model_out=True)
        ref.micro_step += 1
        x_t = engine_q_sample(x0[a:b], t[a:b], noise[a:b])
        out = cus.forward(x_t, t[a:b], yd[a:b])
        assert out.grad_fn is not None and out.dtype == torch.float32
        assert torch.equal(out, r["model_out"])
        seed = torch.empty_like(out)
        dev = [v[a:b].cuda().contiguous() for v in (x0, noise, t)]
        check(lib.latte_debug_loss_grad(cus.diffusion._h, 0, ptr(dev[0]), ptr(x_t), ptr(dev[1]), ptr(out.detach()), ptr(dev[2]), b - a, Fr, C,
                                        H * H, ptr(seed), stream_ptr()))
        out.backward(seed)
        assert cus.micro_step == i + 1
    torch.cuda.synchronize()
    assert float(ref.grads.abs().max()) > 0.0
    assert torch.equal(cus.grads, ref.grads)


# ------------------------------------------------------------------------------------------------ 2. / 3. against the oracle
@pytest.mark.parametrize("dtype", DTYPES)
def test_custom_loss_parameter_gradients_match_the_oracle(dtype):
    want, _, loss_ref = oracle_custom()
    got, _, loss = engine_custom(dtype)
    assert abs(loss - loss_ref) < 1e-4 * abs(loss_ref), (loss, loss_ref)
    assert set(got) == set(want)
    worst = {k: rel(got[k], want[k]) for k in want}
    record(f"custom::{dtype}", worst)
    print(dtype, "custom loss: worst gradient tensor", max(worst, key=worst.get), max(worst.values()))
    bad = {k: round(v, 6) for k, v in worst.items() if not v < GTOL[dtype]}
    assert not bad, bad


@pytest.mark.parametrize("dtype", DTYPES)
def test_input_gradient_matches_the_oracle(dtype):
    """x_t.grad and x_embedder.proj.weight's gradient are formed from the same token gradient: the weight gradient inside the bound
    and x.grad outside it would mean the new kernel is wrong."""
    want, want_dx, _ = oracle_custom()
    got, got_dx, _ = engine_custom(dtype)
    assert got_dx.shape == want_dx.shape and torch.isfinite(got_dx).all()
    k = "x_embedder.proj.weight"
    e_w, e_x = rel(got[k], want[k]), rel(got_dx, want_dx)
    record(f"input_grad::{dtype}", {"x_t.grad": e_x, k: e_w})
    print(dtype, "x.grad rel L2", e_x, "|", k, e_w)
    assert e_w < GTOL[dtype], e_w
    assert e_x < GTOL[dtype], e_x


# ------------------------------------------------------------------------------------------------ 4. accumulation
@pytest.mark.parametrize("dtype", DTYPES)
def test_accumulation_of_two_custom_micro_batches(dtype):
    """A = 2 with two different custom micro-batches (samples 0 - 1, sample 2) = half the sum of the two single-batch gradients, within
    the bound tests/test_train_accum.py uses for the built-in loss (the single-batch bound: fp32 sums of fp32 gradients)."""
    cfg, sd, x0, noise, t, y, drop, yd = inputs()
    w = torch.tensor(WEIGHTS, device="cuda")

    def step(tr, a, b):
        x_t = engine_q_sample(x0[a:b], t[a:b], noise[a:b])
        out = tr.forward(x_t, t[a:b], yd[a:b])
        custom_per_sample(out, noise[a:b].cuda(), w[a:b]).mean().backward()

    singles = []
    for a, b in ((0, 2), (2, 3)):
        tr = trainer(dtype)
        step(tr, a, b)
        singles.append(grads_of(tr))
    tr = trainer(dtype, accum=2)
    step(tr, 0, 2)
    assert tr.micro_step == 1
    step(tr, 2, 3)
    assert tr.micro_step == 2
    got = grads_of(tr)
    worst = {k: rel(got[k], 0.5 * (singles[0][k] + singles[1][k])) for k in got}
    print(dtype, "accumulated custom window: worst", max(worst, key=worst.get), max(worst.values()))
    assert max(worst.values()) < GTOL[dtype], {k: v for k, v in worst.items() if not v < GTOL[dtype]}
    import latte_amd
    with pytest.raises(latte_amd.LatteError):                                   # the window is complete: optimizer_step() is due
        step(tr, 0, 2)
    gn = tr.optimizer_step()
    assert float(gn) > 0 and tr.micro_step == 0


# ------------------------------------------------------------------------------------------------ 5. staged backward
@pytest.mark.parametrize("dtype", DTYPES)
def test_staged_custom_backward_is_bit_identical(dtype):
    plain, plain_dx, _ = engine_custom(dtype)
    staged, staged_dx, _ = engine_custom(dtype, staged=True)
    for k in plain:
        assert torch.equal(plain[k], staged[k]), k
    assert torch.equal(plain_dx, staged_dx)


# ------------------------------------------------------------------------------------------------ 6. train_step(loss_fn=...)
@functools.lru_cache(maxsize=None)
def uncond_case():
    """extras = 1, learn_sigma = False: two keys of TRAIN_STEP changed, weights from lo.init_state_dict; the oracle's gradients of the
    built-in loss (then the plain MSE) once."""
    kw = dict(TRAIN_STEP, extras=1, learn_sigma=False)
    cfg = lo.LatteConfig(**kw)
    sd = lo.init_state_dict(cfg, seed=11)
    _, _, x0, noise, t, _, _, _ = inputs()
    terms, _, grads = to.loss_and_grads(sd, cfg, do.Schedule("", learn_sigma=False), x0, t, noise)
    return kw, sd, terms, grads


@pytest.mark.parametrize("dtype", DTYPES)
def test_train_step_with_a_loss_fn_matches_the_builtin_step_and_the_oracle(dtype):
    """train_step(loss_fn=mse) and the built-in train_step on the same t and noise.  train_step's optimiser step leaves the gradient
    buffer zeroed, so both run as micro-batch 1 of a window of 2: the buffer then holds the gradient / 2, exactly."""
    import latte_amd
    kw, sd, terms, want = uncond_case()
    _, _, x0, noise, t, _, _, _ = inputs()
    res = {}
    for name, fn in (("custom", mse_loss_fn), ("builtin", None)):
        tr = trainer(dtype, accum=2, kw_model=kw, sd=sd, diffusion=latte_amd.create_diffusion("", learn_sigma=False))
        out = tr.train_step(x0, t=t, noise=noise, loss_fn=fn)
        assert out["updated"] is False and "grad_norm" not in out and tr.micro_step == 1
        assert rel(out["loss"].cpu(), terms["loss"]) < 1e-4
        res[name] = {k: 2.0 * v for k, v in grads_of(tr).items()}
        worst = {k: rel(res[name][k], want[k]) for k in want}
        record(f"loss_fn::{name}::{dtype}", worst)
        print(dtype, name, "worst gradient tensor", max(worst, key=worst.get), max(worst.values()))
        bad = {k: round(v, 6) for k, v in worst.items() if not v < GTOL[dtype]}
        assert not bad, (name, bad)
    both = {k: rel(res["custom"][k], res["builtin"][k]) for k in want}
    print(dtype, "custom against built-in: worst", max(both, key=both.get), max(both.values()))
    assert max(both.values()) < GTOL[dtype], {k: v for k, v in both.items() if not v < GTOL[dtype]}


def test_kl_and_xstart_diffusions_need_a_loss_fn():
    import latte_amd
    _, _, x0, noise, t, y, drop, _ = inputs()
    for d in (latte_amd.create_diffusion("", predict_xstart=True), latte_amd.create_diffusion("", use_kl=True)):
        tr = trainer("f16", diffusion=d)
        with pytest.raises(latte_amd.LatteError):
            tr.train_step(x0, y=y, t=t, noise=noise, drop_mask=drop)
        assert tr.micro_step == 0
        out = tr.train_step(x0, y=y, t=t, noise=noise, drop_mask=drop, loss_fn=weighted_loss_fn)
        assert out["updated"] and torch.isfinite(out["loss"]).all() and float(out["grad_norm"]) > 0


# ------------------------------------------------------------------------------------------------ 7. states
def _forward(tr, n=3):
    cfg, sd, x0, noise, t, y, drop, yd = inputs()
    return tr.forward(engine_q_sample(x0[:n], t[:n], noise[:n]), t[:n], yd[:n])


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_graph_at_a_time(dtype):
    import latte_amd
    tr = trainer(dtype, accum=4)
    out = _forward(tr)
    out.sum().backward(retain_graph=True)
    assert tr.micro_step == 1
    with pytest.raises(latte_amd.LatteError):                                   # a second backward
        out.sum().backward()
    assert tr.micro_step == 1
    stale = _forward(tr)
    fresh = _forward(tr)
    with pytest.raises(latte_amd.LatteError):                                   # made stale by a newer forward
        stale.sum().backward()
    fresh.sum().backward()
    assert tr.micro_step == 2
    with torch.no_grad():
        plain = _forward(tr)
    assert plain.grad_fn is None and not plain.requires_grad
    assert torch.equal(plain, fresh)


@pytest.mark.parametrize("dtype", DTYPES)
def test_refused_inputs(dtype):
    import latte_amd
    cfg, sd, x0, noise, t, y, drop, yd = inputs()
    tr = trainer(dtype, max_batch=2)
    x_t = engine_q_sample(x0, t, noise)
    with pytest.raises(latte_amd.LatteError):                                   # batch > max_batch
        tr.forward(x_t, t, yd)
    with pytest.raises(latte_amd.LatteError):                                   # a wrong frame count
        tr.forward(x_t[:2, :3], t[:2], yd[:2])
    with pytest.raises(latte_amd.LatteError):                                   # labels missing on a class-conditional model
        tr.forward(x_t[:2], t[:2])
    out = tr.forward(x_t[:2], t[:2], yd[:2])
    # A gradient of the wrong shape: torch's autograd engine validates every gradient against the output's metadata before it calls a
    # node, so through out.backward() the refusal is torch's own RuntimeError; the trainer's check is what stands behind it
    with pytest.raises((latte_amd.LatteError, RuntimeError)):
        out.backward(torch.ones(2, 4, 8, 8, 9, device="cuda"))
    for bad in (torch.ones(2, 4, 8, 8, 9, device="cuda"), torch.ones(out.shape, device="cuda", dtype=torch.float64), torch.ones(out.shape)):
        with pytest.raises(latte_amd.LatteError):                               # shape, dtype, device
            tr._engine_backward(tr._generation, bad, tuple(out.shape), False)
    assert tr.micro_step == 0
    out.backward(torch.ones_like(out))                                          # a refused gradient does not spend the graph
    assert tr.micro_step == 1


def test_joint_trainer_refuses_joint_batches():
    import latte_amd
    kw = dict(TRAIN_STEP, input_size=16)                                        # 64 tokens per frame: what a joint trainer needs
    cfg = lo.LatteConfig(**kw)
    tr = trainer("f16", max_batch=1, kw_model=kw, sd=lo.init_state_dict(cfg, seed=3), use_image_num=2)
    g = torch.Generator("cpu").manual_seed(5)
    x = torch.randn(1, cfg.num_frames + 2, 4, 16, 16, generator=g).cuda()
    tt, yy = torch.tensor([10]), torch.tensor([1])
    with pytest.raises(latte_amd.LatteError):
        tr.forward(x, tt, yy)
    with pytest.raises(latte_amd.LatteError):
        tr.train_step(x, y=yy, y_image=torch.tensor([[1, 2]]), t=tt, noise=torch.randn_like(x), loss_fn=weighted_loss_fn)
    out = tr.forward(x[:, :cfg.num_frames], tt, yy)                             # its video-only batches take the custom path
    out.square().mean().backward()
    assert tr.micro_step == 1 and float(tr.grads.abs().max()) > 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_builtin_step_after_an_abandoned_forward(dtype):
    """A forward nobody seeds leaves nothing behind: the next train_step moves parameters, moments and EMA exactly as on a fresh trainer."""
    cfg, sd, x0, noise, t, y, drop, yd = inputs()
    res = []
    for abandon in (False, True):
        tr = trainer(dtype)
        if abandon:
            out = _forward(tr, 2)
            assert out.grad_fn is not None
        o = tr.train_step(x0, y=y, t=t, noise=noise, drop_mask=drop)
        assert o["updated"]
        torch.cuda.synchronize()
        res.append([b.clone() for b in (tr.params, tr.exp_avg, tr.exp_avg_sq, tr.ema, o["loss"])])
        if abandon:
            import latte_amd
            with pytest.raises(latte_amd.LatteError):                           # the built-in step made it stale
                out.sum().backward()
    for a, b in zip(*res):
        assert torch.equal(a, b)
    assert float(res[0][1].abs().max()) > 0.0


# ------------------------------------------------------------------------------------------------ 8. a short run
@pytest.mark.parametrize("dtype", DTYPES)
def test_ten_steps_of_the_weighted_loss_lower_it(dtype):
    cfg, sd, x0, noise, t, y, drop, yd = inputs()
    tr = trainer(dtype, lr=1e-3)
    losses = []
    for _ in range(10):
        out = tr.train_step(x0, y=y, t=t, noise=noise, drop_mask=drop, loss_fn=weighted_loss_fn)
        assert out["updated"] and float(out["grad_norm"]) > 0
        losses.append(float(out["loss"].mean()))
    assert all(l == l for l in losses) and losses[-1] < losses[0], losses
    assert tr.train_steps == 10 and tr.scaler_state()["skipped_updates"] == 0.0


# ------------------------------------------------------------------------------------------------ the training driver's `loss_fn:` key
def test_train_driver_takes_a_loss_fn(tmp_path):
    """tools/train.py with `loss_fn: "module:function"` in the config: resolves it, logs its name, trains and writes a checkpoint."""
    import subprocess
    import sys
    cfg = open(os.path.join(ROOT, "configs", "tiny_train.yaml")).read()
    cfg = cfg.replace("max_train_steps: 8", "max_train_steps: 4").replace("log_every: 4", "log_every: 2")
    path = tmp_path / "custom.yaml"
    path.write_text(cfg + 'loss_fn: "test_train_custom_host:eps_mse"\n')
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "tests"), os.environ.get("PYTHONPATH", "")]))
    out = str(tmp_path / "run")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "train.py"), "--config", str(path), "--out", out], capture_output=True,
                       text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Custom loss: test_train_custom_host:eps_mse" in r.stdout, r.stdout
    assert r.stdout.count("Train Loss") == 2 and "Saved checkpoint" in r.stdout, r.stdout
    assert os.path.isfile(os.path.join(out, "checkpoints", "0000004.pt"))
