"""Joint image-video training, CPU side: the fp32 restatement (tests/joint_reference.py) against the committed fixture of what the
reference objects computed (tests/golden/train_joint.npz, tools/make_joint_golden.py) and against the live reference where it is
present; the decomposition the engine's joint step rests on; the driver's host-side pieces."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import diffusion_oracle as do
from oracle import reference_loader as rl
from oracle import train_oracle as to

import joint_reference as jr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "train_joint.npz")

# The restatement runs the reference's operations in the reference's order: on the machine that wrote the fixture it reproduces terms,
# model output and every gradient to the bit (measured: 0.0).  What differs between machines is the order of the fp32 sums inside
# BLAS; a direct measure of that sensitivity on these tensors is the decomposition below, the same sums in another order: 6.5e-7
# worst relative L2 per gradient tensor (4.8e-7 on a smaller model).  One order of magnitude over it:
REF_TOL = 5e-6
# the decomposition itself (video pass + image pass against the joint graph): measured 6.5e-7 (gradients), 1.2e-7 (terms); the same margin
DEC_TOL = 5e-6


def rel(a, b):
    return float((a - b).norm() / (b.norm() + 1e-30))


@pytest.fixture(scope="module")
def joint():
    cfg, sd, x0, noise, t, y, yi, drop, idrop = jr.joint_inputs()
    terms, out, grads = jr.joint_loss_and_grads(sd, cfg, do.Schedule(""), x0, t, noise, y, yi, drop, idrop)
    return (cfg, sd, x0, noise, t, y, yi, drop, idrop), terms, out, grads


def test_fixture_is_small_and_numeric():
    assert os.path.getsize(GOLD) < 1 << 20
    z = np.load(GOLD, allow_pickle=False)
    assert all(z[k].dtype.kind in "fiu" for k in z.files)


def test_restatement_matches_reference_fixture(joint):
    _, terms, out, grads = joint
    z = np.load(GOLD)
    for k in ("loss", "mse", "vb"):
        assert torch.allclose(terms[k], torch.from_numpy(z[f"terms::{k}"]), rtol=REF_TOL, atol=1e-7), k
    assert rel(out, torch.from_numpy(z["model_out"])) < REF_TOL
    keys = {k[len("gnorm::"):] for k in z.files if k.startswith("gnorm::")}
    assert keys == set(grads)
    for k, g in grads.items():
        want = torch.from_numpy(z[f"gsample::{k}"])
        assert want.numel() == min(g.numel(), jr.GOLD_SAMPLE)
        assert rel(g.reshape(-1)[jr.sample_index(g.numel())], want) < REF_TOL, k
        assert abs(float(g.double().norm()) - float(z[f"gnorm::{k}"])) < REF_TOL * float(z[f"gnorm::{k}"]), k
    # sample 1's image labels were dropped, sample 2's video label: the null row holds both; class 3 comes from images alone
    gy = grads["y_embedder.embedding_table.weight"]
    assert all(float(gy[r].abs().max()) > 0 for r in (0, 1, 3, 4, 5))


@pytest.mark.skipif(not rl.reference_available(), reason="reference checkout not present")
@pytest.mark.parametrize("extras", [1, 2])
def test_restatement_matches_live_reference(extras, monkeypatch):
    # the timm stand-in and the reference modules leave sys.modules with the test (other tests probe for the real timm)
    for name in ("timm", "timm.models", "timm.models.vision_transformer", "_reference_latte_img", "_reference_diffusion"):
        if name not in sys.modules:
            monkeypatch.setitem(sys.modules, name, None)
            del sys.modules[name]
    model = dict(jr.J_MODEL, depth=2, extras=extras)
    cfg, sd, x0, noise, t, y, yi, drop, idrop = jr.joint_inputs(model, images=2, batch=2, weight_seed=5)
    terms_r, out_r, grads_r = jr.reference_step(model, sd, x0, noise, t, y, yi, drop, idrop, 2)
    terms, out, grads = jr.joint_loss_and_grads(sd, cfg, do.Schedule(""), x0, t, noise, y, yi, drop, idrop, images=2)
    # LatteIMG holds exactly Latte's parameters: the state dict loaded above without a missing or unexpected key
    assert set(grads) == set(grads_r)
    for k in terms_r:
        assert torch.allclose(terms[k], terms_r[k], rtol=REF_TOL, atol=1e-7), k
    assert rel(out, out_r) < REF_TOL
    for k in grads:
        assert rel(grads[k], grads_r[k]) < REF_TOL, k


def test_decomposition_into_a_video_pass_and_an_image_pass(joint):
    (cfg, sd, x0, noise, t, y, yi, drop, idrop), terms, out, grads = joint
    Fr, N = cfg.num_frames, jr.J_IMAGES
    s = do.Schedule("")
    tv, ov, gv = to.loss_and_grads(sd, cfg, s, x0[:, :Fr], t, noise[:, :Fr], y, drop)            # the step the trainer already runs
    ti, oi, gi = jr.image_pass(sd, cfg, s, x0[:, Fr:], t, noise[:, Fr:], yi, idrop)
    wv, wi = jr.loss_weights(Fr, N)
    for k in ("loss", "mse", "vb"):
        merged = (Fr * tv[k] + ti[k].reshape(-1, N).sum(1)) / (Fr + N)
        assert torch.allclose(merged, terms[k], rtol=DEC_TOL, atol=1e-7), k
    assert rel(torch.cat([ov, oi.reshape(-1, N, *oi.shape[2:])], dim=1), out) < DEC_TOL
    for k in grads:
        assert rel(wv * gv[k] + wi * gi[k], grads[k]) < DEC_TOL, k
    for k in grads:                                                                              # images never reach a temporal block
        if k.startswith(("blocks.1.", "blocks.3.")):
            assert float(gi[k].abs().max()) == 0.0, k
            assert rel(wv * gv[k], grads[k]) < DEC_TOL, k


def test_driver_name_mapping_frame_draw_and_loss_weights():
    from latte_amd.train_util import data_seed, draw_image_frames, joint_loss_weights, latte_preset_name
    assert latte_preset_name("LatteIMG-XL/2") == "Latte-XL/2"
    assert latte_preset_name("LatteIMG-S/8") == "Latte-S/8"
    assert latte_preset_name("Latte-B/2") == "Latte-B/2"
    assert latte_preset_name("LatteT2V") == "LatteT2V"

    def draw(step):
        return draw_image_frames(37, 4, 8, torch.Generator("cpu").manual_seed(data_seed(3407, step, 0, 1, 0, 1)))
    a, b = draw(5), draw(5)
    assert a.shape == (4, 8) and a.dtype == torch.int64 and torch.equal(a, b)                      # a resumed run redraws the same frames
    assert int(a.min()) >= 0 and int(a.max()) < 37
    assert not torch.equal(a, draw(6))
    with pytest.raises(ValueError):
        draw_image_frames(0, 4, 8, torch.Generator("cpu"))

    wv, wi = joint_loss_weights(16, 8)
    assert wv == 16 / 24 and wi == 8 / 24 and joint_loss_weights(4, 0) == (1.0, 0.0)
    assert (wv, wi) == jr.loss_weights(16, 8)
    # the engine multiplies the pass weights into the loss divisor: (F + N) / F and (F + N) / N, whose inverses are these
    assert abs(1.0 / ((16 + 8) / 16) - wv) < 1e-15 and abs(1.0 / ((16 + 8) / 8) - wi) < 1e-15


def test_configs_name_the_joint_keys():
    import latte_amd
    for name, n in (("ffs_img_train.yaml", 8), ("tiny_img_train.yaml", 2)):
        args = latte_amd.load_config(os.path.join(ROOT, "configs", name))
        assert int(args.use_image_num) == n and str(args.model).startswith("LatteIMG-")
        assert int(args.use_image_num) <= int(args.num_frames)
        patch = int(str(args.model).split("/")[1])
        assert ((int(args.image_size) // 8 // patch) ** 2) % 64 == 0
        assert "frame_data_path" in args


def test_get_models_keeps_refusing_the_latteimg_names():
    import latte_amd
    args = latte_amd.load_config(os.path.join(ROOT, "configs", "tiny_img_train.yaml"))
    args.latent_size = 16
    with pytest.raises(Exception):
        latte_amd.get_models(args)
