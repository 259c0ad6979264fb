"""A/B of two builds of the library, or of two trees with their front ends, on the trainer: every path of the training step on fixed
seeds, sha256 of every returned tensor.

  python tools/train_ab.py --out profiles/trainer_refactor_head.json                                    # the tree's library
  LATTE_AMD_LIB=<other build>.so python tools/train_ab.py --out profiles/trainer_refactor_parent.json   # another build
  python tools/train_ab.py --tree <built checkout of another commit> --out ...                          # library AND front end
  python tools/train_ab.py --compare profiles/trainer_refactor_parent.json profiles/trainer_refactor_head.json
  python tools/train_ab.py --only A::f16::fuse_small1::batch3 --out one.json                            # one case

Builds nothing: it loads LATTE_AMD_LIB or latte_amd/lib/liblatte_amd.so of the tree ``latte_amd``, ``oracle`` and ``tests/`` are
imported from (--tree, default this one).  Models:
  A   oracle.make_golden.TRAIN_STEP (depth 2, D 128, 2 heads, 4 frames x 16 tokens, class-conditional, learned sigma): the GELU passes are
      separate launches (mlp_hidden 512 is no multiple of 192)
  B   depth 2, D 384, 6 heads, input_size 8, 4 frames, extras 1: mlp_hidden 1536, the GELU-epilogue GEMMs run
  J   the fixture and use_image_num of tests/test_train_joint.py (tests/joint_reference.py)
Cases:
  A x {f16, bf16} x fuse_small {1, 0} at batch 3 and batch 9 (the finalize kernels' second pass of eight samples)
  B x f16 x fuse_small {1, 0} x fuse_gelu {1, 0}
  A, fuse_small 1, debug choice tn_kernel 4: the folded path's separate launch_colsum_half launches
  A, gradient accumulation over two micro-batches, both fuse_small
  J, a joint micro-batch, both fuse_small
  A, the custom path (forward, a caller's seed, the stages, latte_trainer_input_grad), both fuse_small
  A, the staged path (begin + stages, every latte_trainer_stage_range recorded), both fuse_small
  A with LoRA adapters (rank 8, B seeded nonzero so that A receives a gradient on the first step), both fuse_small: all four targets on
     the built-in step, two accumulated micro-batches, the staged path and the custom path; targets qkv,fc2 on the built-in step.  These
     hash the ADAPTER buffers where the other cases hash the base's, and the base parameter buffer, which must not move
  A, plain and LoRA: ``training_state()`` after one optimiser step and one micro-batch of the next window, keys walked in sorted order
Every case hashes the loss terms, the model output copy and the flat gradient buffer; then, after optimizer_step, the parameters, both
moments, the EMA and the eight scaler fields; then the gradient buffer of a second forward_backward (the re-packed weights).
The label-table gradient is a scatter with atomic adds: labels and drop masks are chosen so that no table row, the null class
included, receives more than two addends (two commute exactly, three need not) -- where the writers ADD to what an earlier pass left
(the second micro-batch of a window, the image pass), that earlier value counts as one.  Two runs agree when every hash agrees."""
import argparse
import hashlib
import json
import os
import sys

import torch

_pre = argparse.ArgumentParser(add_help=False)
_pre.add_argument("--tree")
ROOT = os.path.abspath(_pre.parse_known_args()[0].tree or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import latte_amd  # noqa: E402
from latte_amd import _lib  # noqa: E402
from latte_amd._lib import check, load_library  # noqa: E402

A_MODEL = dict(depth=2, hidden_size=128, patch_size=2, num_heads=2, input_size=8, num_frames=4, num_classes=5, extras=2, learn_sigma=True)
B_MODEL = dict(depth=2, hidden_size=384, patch_size=2, num_heads=6, input_size=8, num_frames=4, extras=1, learn_sigma=True)


def sha(t):
    """sha256 of the tensor's bytes; a tensor with a non-finite element is marked, so that a step that left the fp32 range shows"""
    torch.cuda.synchronize()
    t = t.detach().cpu().contiguous()
    return ("" if bool(torch.isfinite(t).all()) else "nonfinite:") + hashlib.sha256(t.numpy().tobytes()).hexdigest()


def inputs_a(batch, seed):
    """-> kw, sd, (x0, noise, t, y, drop) of model A, the fixture's weights (through tests/: the tools do not import the oracle).  Table
    rows of the labels after dropout: batch 3 -> 1, 4, null; batch 9 -> 0 0 1 1 2 3 4 null null."""
    import test_training_step as ts
    cfg, sd = ts.train_step_inputs()[:2]
    assert all(getattr(cfg, k) == v for k, v in A_MODEL.items()), cfg     # A_MODEL restates oracle.make_golden.TRAIN_STEP
    g = torch.Generator("cpu").manual_seed(seed)
    x0 = (torch.randn(batch, 4, 4, 8, 8, generator=g) * 0.6).clamp(-1.0, 1.0)
    noise = torch.randn(batch, 4, 4, 8, 8, generator=g)
    t = torch.tensor([0, 500, 999, 250, 750, 1, 37, 640, 900][:batch], dtype=torch.int64)
    y = torch.tensor([1, 4, 2, 0, 1, 0, 3, 2, 3][:batch], dtype=torch.int64)
    drop = torch.tensor([False, False, True, False, False, False, False, False, True][:batch])
    return A_MODEL, sd, (x0, noise, t, y, drop)


def inputs_b(batch, seed):
    import joint_reference as jr
    sd = jr.joint_inputs(B_MODEL, images=0, batch=1, weight_seed=12)[1]      # the oracle's synthetic weights, seed 12
    g = torch.Generator("cpu").manual_seed(seed)
    x0 = (torch.randn(batch, 4, 4, 8, 8, generator=g) * 0.6).clamp(-1.0, 1.0)
    noise = torch.randn(batch, 4, 4, 8, 8, generator=g)
    return B_MODEL, sd, (x0, noise, torch.tensor([0, 500, 999][:batch], dtype=torch.int64), None, None)


def make_trainer(kw, sd, max_batch, dtype, fuse_small, fuse_gelu=1, **tkw):
    model = latte_amd.Latte(**kw)
    model.load_state_dict(sd)
    tr = latte_amd.LatteTrainer(model.to("cuda"), latte_amd.create_diffusion(""), max_batch=max_batch, compute_dtype=dtype,
                                start_clip_iter=0, **tkw)        # start_clip_iter 0: the clip coefficient is applied
    tr.set_option("fuse_small", fuse_small)
    tr.set_option("fuse_gelu", fuse_gelu)
    return tr


def after_step(tr, rec, again):
    """optimizer_step, the whole optimiser state, then the gradients of a second pass on the re-packed weights"""
    rec["grad_norm"] = sha(tr.optimizer_step())
    rec.update(params=sha(tr.params), exp_avg=sha(tr.exp_avg), exp_avg_sq=sha(tr.exp_avg_sq), ema=sha(tr.ema))
    rec["scaler"] = [float(v).hex() for v in tr.scaler_state().values()]
    out = again()
    rec.update(grads_2=sha(tr.grads), loss_2=sha(out["loss"]))
    return rec


def terms(out, rec, tag=""):
    for k in ("loss", "mse", "vb", "model_out"):
        if k in out:
            rec[k + tag] = sha(out[k])


def plain(kw, sd, inp, dtype, fuse_small, fuse_gelu=1, staged=False):
    x0, noise, t, y, drop = inp
    tr = make_trainer(kw, sd, x0.shape[0], dtype, fuse_small, fuse_gelu)
    rec = {}
    if staged:   # every stage's slice of the gradient buffer, as the data-parallel driver asks for it
        lib = load_library()
        rec["stage_ranges"] = []
        for k in range(lib.latte_trainer_num_stages(tr._h)):
            off, n = _lib.c_i64(), _lib.c_i64()
            check(lib.latte_trainer_stage_range(tr._h, k, off, n))
            rec["stage_ranges"].append([off.value, n.value])
    run = lambda: tr.forward_backward(x0, t, noise, y, drop, return_model_out=True, overlap_all_reduce=staged)   # noqa: E731
    terms(run(), rec)
    rec["grads"] = sha(tr.grads)
    return after_step(tr, rec, run)


def accumulated(kw, sd, inp, fuse_small):
    """A window of two micro-batches; the second one's labels hit three different table rows (each adds ONE value to what is there)"""
    x0, noise, t, y, drop = inp
    tr = make_trainer(kw, sd, x0.shape[0], "f16", fuse_small, gradient_accumulation_steps=2)
    g = torch.Generator("cpu").manual_seed(77)
    x1 = (torch.randn(x0.shape, generator=g) * 0.6).clamp(-1.0, 1.0)
    n1 = torch.randn(x0.shape, generator=g)
    t1, y1 = torch.tensor([3, 420, 998]), torch.tensor([0, 3, 2])
    rec = {}

    def window(tag=""):
        out, last = tr.backward_micro_batch(x0, t, noise, y, drop)
        assert not last
        terms(out, rec, "::micro1" + tag)
        rec["grads::micro1" + tag] = sha(tr.grads)
        out, last = tr.backward_micro_batch(x1, t1, n1, y1, None)
        assert last
        return out
    terms(window(), rec, "::micro2")
    rec["grads"] = sha(tr.grads)
    return after_step(tr, rec, lambda: window("::window2"))


def joint(fuse_small):
    """Fixture J with labels of its own: the video pass assigns rows 1, 4, 2 one value each, the image pass adds one more to each of
    them and two to each of rows 0, 3 and null"""
    import joint_reference as jr
    cfg, sd, x0, noise, t, _, _, _, _ = jr.joint_inputs()
    y = torch.tensor([1, 4, 2])
    yi = torch.tensor([[1, 0, 0], [4, 3, 3], [2, cfg.num_classes, cfg.num_classes]])
    tr = make_trainer(jr.J_MODEL, sd, x0.shape[0], "f16", fuse_small, use_image_num=jr.J_IMAGES)
    rec = {}
    run = lambda: tr.forward_backward(x0, t, noise, y, None, return_model_out=True, y_image=yi)   # noqa: E731
    terms(run(), rec)
    rec["grads"] = sha(tr.grads)
    return after_step(tr, rec, run)


def custom(kw, sd, inp, fuse_small):
    """forward, a caller's seed, the stages, the input gradient"""
    x0, noise, t, y, drop = inp
    tr = make_trainer(kw, sd, x0.shape[0], "f16", fuse_small)
    rec = {}

    def run():
        x = x0.cuda().requires_grad_(True)
        out = tr.forward(x, t, y, drop)
        seed = torch.randn(out.shape, generator=torch.Generator("cpu").manual_seed(5)) * 1e-4
        out.backward(seed.cuda())
        return {"loss": x.grad, "model_out": out}
    out = run()
    rec.update(model_out=sha(out["model_out"]), input_grad=sha(out["loss"]), grads=sha(tr.grads))
    return after_step(tr, rec, run)


def seeded_adapters(tr, seed=41):
    """A ~ U(+-1 / sqrt(K)) and a NONZERO B ~ N(0, 0.02) from a fixed seed, in the trainer's table order"""
    g = torch.Generator("cpu").manual_seed(seed)
    return {k: (torch.rand(v.shape, generator=g) * 2 - 1) * v.shape[1] ** -0.5 if k.endswith(".lora_A") else
            torch.randn(v.shape, generator=g) * 0.02 for k, v in tr.lora_state_dict().items()}


def lora(kw, sd, inp, fuse_small, path, targets="qkv,proj,fc1,fc2"):
    """path: "step" (forward_backward), "accumulate2", "staged" or "custom" -- the plain cases' paths on a rank-8 LoRA trainer"""
    x0, noise, t, y, drop = inp
    tr = make_trainer(kw, sd, x0.shape[0], "f16", fuse_small, lora_rank=8, lora_alpha=16.0, lora_targets=targets,
                      gradient_accumulation_steps=2 if path == "accumulate2" else 1)
    tr.load_lora_state_dict(seeded_adapters(tr))
    rec = {}
    if path == "staged":
        lib = load_library()
        rec["stage_ranges"] = []
        for k in range(lib.latte_trainer_num_stages(tr._h)):
            off, n = _lib.c_i64(), _lib.c_i64()
            check(lib.latte_trainer_stage_range(tr._h, k, off, n))
            rec["stage_ranges"].append([off.value, n.value])

    def run(tag=""):
        if path == "custom":
            x = x0.cuda().requires_grad_(True)
            out = tr.forward(x, t, y, drop)
            out.backward((torch.randn(out.shape, generator=torch.Generator("cpu").manual_seed(5)) * 1e-4).cuda())
            return {"loss": x.grad, "model_out": out}
        if path == "accumulate2":
            out, last = tr.backward_micro_batch(x0, t, noise, y, drop)
            assert not last
            terms(out, rec, "::micro1" + tag)
            rec["lora_grads::micro1" + tag] = sha(tr.lora_grads)
            out, last = tr.backward_micro_batch(x0.flip(0), t.flip(0), noise.flip(0), torch.tensor([0, 3, 2]), None)
            assert last
            return out
        return tr.forward_backward(x0, t, noise, y, drop, return_model_out=True, overlap_all_reduce=path == "staged")
    terms(run(), rec)
    rec["lora_grads"] = sha(tr.lora_grads)
    rec["grad_norm"] = sha(tr.optimizer_step())
    rec.update(lora_params=sha(tr.lora_params), lora_exp_avg=sha(tr.lora_exp_avg), lora_exp_avg_sq=sha(tr.lora_exp_avg_sq),
               lora_ema=sha(tr.lora_ema), params=sha(tr.params))
    rec["scaler"] = [float(v).hex() for v in tr.scaler_state().values()]
    out = run("::window2")
    rec.update(lora_grads_2=sha(tr.lora_grads), loss_2=sha(out["loss"]))
    return rec


def state_sha(kw, sd, inp, lora_rank):
    """sha256 over ``training_state()`` inside the second window of two micro-batches: keys in sorted order, tensors by their bytes"""
    x0, noise, t, y, drop = inp
    tkw = dict(lora_rank=lora_rank, lora_alpha=16.0) if lora_rank else {}
    tr = make_trainer(kw, sd, x0.shape[0], "f16", 1, gradient_accumulation_steps=2, **tkw)
    if lora_rank:
        tr.load_lora_state_dict(seeded_adapters(tr))
    for _ in range(3):
        tr.train_step(x0, y=y, t=t, noise=noise, drop_mask=drop)
    torch.cuda.synchronize()
    h, keys = hashlib.sha256(), []

    def walk(v, path):
        if isinstance(v, dict):
            for k in sorted(v):
                walk(v[k], path + "/" + str(k))
            return
        keys.append(path)
        h.update(path.encode())
        h.update(v.detach().cpu().contiguous().numpy().tobytes() if torch.is_tensor(v) else
                 (float(v).hex() if isinstance(v, float) else repr(v)).encode())
    walk(tr.training_state(), "")
    return {"training_state": h.hexdigest(), "entries": len(keys), "top": sorted({k.split("/")[1] for k in keys})}


def cases():
    """name -> thunk"""
    c = {}
    for dtype in ("f16", "bf16"):
        for fs in (1, 0):
            for batch in (3, 9):
                c[f"A::{dtype}::fuse_small{fs}::batch{batch}"] = lambda d=dtype, f=fs, b=batch: plain(*inputs_a(b, 31), d, f)
    for fs in (1, 0):
        for fg in (1, 0):
            c[f"B::f16::fuse_small{fs}::fuse_gelu{fg}"] = lambda f=fs, g=fg: plain(*inputs_b(3, 32), "f16", f, g)

    def tn4():
        lib = load_library()
        check(lib.latte_debug_set_choice(b"tn_kernel", 4))
        try:
            return plain(*inputs_a(3, 31), "f16", 1)
        finally:
            check(lib.latte_debug_set_choice(b"tn_kernel", 0))
    c["A::f16::fuse_small1::batch3::tn_kernel4"] = tn4
    for fs in (1, 0):
        c[f"A::accumulate2::fuse_small{fs}"] = lambda f=fs: accumulated(*inputs_a(3, 31), f)
        c[f"J::joint::fuse_small{fs}"] = lambda f=fs: joint(f)
        c[f"A::custom::fuse_small{fs}"] = lambda f=fs: custom(*inputs_a(3, 31), f)
        c[f"A::staged::fuse_small{fs}"] = lambda f=fs: plain(*inputs_a(3, 31), "f16", f, staged=True)
        for path in ("step", "accumulate2", "staged", "custom"):
            c[f"A::lora8::{path}::fuse_small{fs}"] = lambda f=fs, p=path: lora(*inputs_a(3, 31), f, p)
        c[f"A::lora8::qkv,fc2::step::fuse_small{fs}"] = lambda f=fs: lora(*inputs_a(3, 31), f, "step", "qkv,fc2")
    c["A::training_state::plain"] = lambda: state_sha(*inputs_a(3, 31), 0)
    c["A::training_state::lora8"] = lambda: state_sha(*inputs_a(3, 31), 8)
    return c


def compare(a, b):
    ra, rb = (json.load(open(p))["cases"] for p in (a, b))
    bad = sorted(k for k in set(ra) | set(rb) if ra.get(k) != rb.get(k))
    print(f"{len(ra)} / {len(rb)} cases, {len(bad)} differ")
    for k in bad:
        fa, fb = ra.get(k) or {}, rb.get(k) or {}
        print("  " + k + ": " + ", ".join(sorted(f for f in set(fa) | set(fb) if fa.get(f) != fb.get(f))))
    return 1 if bad or not ra else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2, metavar="JSON")
    ap.add_argument("--tree", help="the built checkout to import latte_amd, oracle and tests/ from (default: this one)")
    ap.add_argument("--only", action="append", help="run this case alone (repeatable)")
    a = ap.parse_args()
    if a.compare:
        raise SystemExit(compare(*a.compare))
    if not torch.cuda.is_available():
        raise SystemExit("tools/train_ab.py needs an MI355X")
    if not a.out:
        raise SystemExit("--out or --compare")
    todo = cases()
    if a.only:
        todo = {k: todo[k] for k in a.only}
    done = {}
    for k, fn in todo.items():
        done[k] = fn()
        print(k, flush=True)
    result = {"what": "sha256 of every tensor a training step returns or updates, fixed seeds (tools/train_ab.py)",
              "library": "LATTE_AMD_LIB" if os.environ.get("LATTE_AMD_LIB") else "tree", "version": load_library().latte_version().decode(),
              "device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName, "cases": done}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(done)} cases -> {a.out}")


if __name__ == "__main__":
    main()
