"""The fp32 restatement of likelihood evaluation (tests/bpd_reference.py) against the committed fixture tests/golden/bpd.npz --
what the reference's calc_bpd_loop / _vb_terms_bpd / _prior_bpd computed (tools/make_bpd_golden.py) -- and, where the reference
checkout is present, against the live reference.  CPU only; the GPU tests (test_bpd_kernels.py, test_bpd_loop.py) compare the engine
with the same fixture."""
import os
import sys

import numpy as np
import pytest
import torch

import bpd_reference as br
from _util import GOLDEN
from oracle import diffusion_oracle as do
from oracle.reference_loader import reference_available

TOL = 1e-6   # fp32 against fp32, the same operations in the same order


def _golden():
    return np.load(os.path.join(GOLDEN, "bpd.npz"))


def _rel(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float((np.abs(got - want) / np.maximum(np.abs(want), 1e-30)).max())


def test_input_checksums_match():
    """The seeded CPU generators still give the inputs the fixture was computed on: a miss here is "inputs differ", not a parity miss."""
    z = _golden()
    sums = br.input_checksums()
    assert {k for k in z.files if k.startswith("in::")} == set(sums)
    for k, v in sums.items():
        assert np.array_equal(v, z[k]), k


def test_fixture_holds_numbers_only_and_covers_the_grid():
    z = _golden()
    keys = {br.kernel_key(tag, clip, spec, shape, i) for tag in br.K_TYPES for clip in (True, False) for spec, shape, i in br.kernel_grid()}
    assert keys <= set(z.files)
    assert all(z[k].dtype.kind == "f" and z[k].size <= 128 for k in z.files)
    assert os.path.getsize(os.path.join(GOLDEN, "bpd.npz")) < 256 << 10
    # the reference's t = T-1 eps-MSE of fixture M without clipping is near 2 (an untrained model's eps against a unit normal):
    # the interval of test_bpd_loop's statistical check is this value +- 50 %
    assert 1.0 < float(z["M::clip0::mse"][:, 0].mean()) < 3.0


@pytest.mark.parametrize("clip", [True, False])
def test_model_level_restatement_equals_fixture(clip):
    z = _golden()
    r = br.model_restatement(clip_denoised=clip)
    for k in br.TABLES:
        assert r[k].shape == z[f"M::clip{int(clip)}::{k}"].shape
        assert _rel(r[k].numpy(), z[f"M::clip{int(clip)}::{k}"]) < TOL, k
    assert torch.equal(r["total_bpd"], r["vb"].sum(dim=1) + r["prior_bpd"])


@pytest.mark.parametrize("tag", sorted(br.K_TYPES))
def test_kernel_level_restatement_equals_fixture(tag):
    z = _golden()
    for spec, shape, index in br.kernel_grid():
        s = do.Schedule(spec, **br.K_TYPES[tag])
        x0, nz, x_t, mo = br.kernel_inputs(s, shape, index)
        assert float(x0.max()) == 1.0 and float(x0.min()) == -1.0 and bool((x0 == 0.9995).any()) and bool((x0 == -0.9995).any())
        for clip in (True, False):
            vb, xm, m, _ = br.bpd_terms(s, mo, x0, x_t, nz, index, clip)
            want = z[br.kernel_key(tag, clip, spec, shape, index)]
            assert _rel(torch.stack([vb, xm, m]).numpy(), want) < TOL, (tag, spec, shape, index, clip)
        if tag == "eps_learned":
            assert _rel(br.prior_bpd(s, x0).numpy(), z[f"K::prior::{spec or 'full'}::{shape[0]}x{shape[1]}"]) < TOL


@pytest.mark.skipif(not reference_available(), reason="the reference checkout is present only where the fixture is generated")
def test_restatement_equals_live_reference(monkeypatch):
    """The reference's own calc_bpd_loop with torch.manual_seed set, so both sides consume the same draws (gd:837)."""
    # the timm stand-in and the reference modules leave sys.modules with the test (other tests probe for the real timm)
    for name in ("timm", "timm.models", "timm.models.vision_transformer", "_reference_latte", "_reference_diffusion"):
        if name not in sys.modules:
            monkeypatch.setitem(sys.modules, name, None)
            del sys.modules[name]
    from oracle import reference_loader as rl
    rd, rlatte = rl.load_reference_diffusion(), rl.load_reference_latte()
    kw, cfg, sd, x0, y, noise = br.model_inputs()
    model = rlatte.Latte(**kw)
    model.load_state_dict(sd)
    model.eval()
    torch.manual_seed(br.M_NOISE_SEED)
    with torch.no_grad():
        want = rd.create_diffusion(br.M_SPEC).calc_bpd_loop(model, x0, clip_denoised=True, model_kwargs=dict(y=y))
    got = br.model_restatement(clip_denoised=True)
    for k in br.TABLES:
        assert _rel(got[k].numpy(), want[k].numpy()) < TOL, k
