"""The fp32 restatement of DDIM inversion (tests/invert_reference.py) against the committed fixture tests/golden/invert.npz -- what the
reference's own ddim_reverse_sample computed (tools/make_invert_golden.py) -- and, where the reference checkout is present, against
the live reference; and the alphas_cumprod_next table of the library against the reference's.  CPU only; the GPU tests
(test_invert_kernels.py, test_invert_loop.py) compare the engine with the same fixture.

The kernel-level cases are elementwise fp32 arithmetic: equal bits, on one CPU thread on both sides (invert_reference.one_thread)
and in the child of _util.pinned.

The 50-step chains of fixture M run 50 forwards through MKL.  Where the fixture was written, the restatement reproduces the reference's
chain bit for bit on MKL's default code path; that path depends on the CPU, and on another host the same restatement differed from
the fixture in the seventh digit.  So the fixture is computed on MKL's vendor-neutral path and the restatement runs in the child of
_util.pinned that reproduces it on every x86 host -- and on that path the oracle's GEMMs and the reference's round differently, so
what holds everywhere is 1e-6 relative L2 on every stored sample (measured: 6.8e-8 after step 0 to 7.4e-7 after step 49 of the
guided chain), not equal bits.  The last pred_xstart is a 157-fold amplified difference of samples 48 and 49 (1.3e-5 to 7.2e-5 here);
it is held, element by element, to what those two samples' differences explain, as in tests/test_invert_loop.py."""
import os
import sys

import numpy as np
import pytest
import torch

import invert_reference as ir
from _util import GOLDEN, pinned
from oracle import diffusion_oracle as do
from oracle.reference_loader import reference_available

SPECS = ("", "250", "ddim50", "10,15,20")


def _golden():
    return np.load(os.path.join(GOLDEN, "invert.npz"))


def test_input_checksums_match():
    """The seeded CPU generators still give the inputs the fixture was computed on: a miss here is "inputs differ", not a parity miss."""
    z = _golden()
    sums = ir.input_checksums()
    assert {k for k in z.files if k.startswith("in::")} == set(sums)
    for k, v in sums.items():
        assert np.array_equal(v, z[k]), k


def test_fixture_holds_numbers_only_and_covers_the_grid():
    z = _golden()
    keys = {ir.kernel_key(tag, clip, spec, shape, i) for tag in ir.K_TYPES for clip in (True, False) for spec, shape, i in ir.kernel_grid()}
    assert keys | {k + "::sums" for k in keys} <= set(z.files)
    assert {(spec, i) for spec, _, i in ir.kernel_grid()} == {("50", 0), ("50", 1), ("50", 25), ("50", 48), ("50", 49), ("", 0), ("", 999)}
    assert all(z[k].dtype.kind == "f" for k in z.files)
    assert all(z[k].shape == (2, ir.K_KEEP) and z[k + "::sums"].shape == (2, 2) for k in keys)
    for case in ir.M_CASES:
        B = 4 if case == "guided" else 2
        assert z[f"M::{case}::sample"].shape == (len(ir.M_CHECKPOINTS), B, 4, 4, 8, 8) and z[f"M::{case}::pred_xstart"].shape == (B, 4, 4, 8, 8)
        assert np.isfinite(z[f"M::{case}::sample"]).all()
    assert np.abs(z["M::clip1::pred_xstart"]).max() <= 1.0 < np.abs(z["M::clip0::pred_xstart"]).max()
    assert os.path.getsize(os.path.join(GOLDEN, "invert.npz")) < 1 << 20


TOL = 1e-6            # fp32 against fp32, the same operations in the same order; GEMMs blocked differently
X0_ROUNDING = 2e-4    # fp32 rounding of 157.4 x - 157.4 eps at |x|, |eps| <= 4 (tests/test_invert_loop.py)


def _rel_l2(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def _model_restatement(case):
    r = ir.model_restatement(case)
    return r["sample"], r["pred_xstart"]


def _check_chain(sample, x0, want_sample, want_x0):
    err = [_rel_l2(sample[j], want_sample[j]) for j in range(len(ir.M_CHECKPOINTS))]
    assert max(err) < TOL, err
    s = do.Schedule(ir.M_SPEC)
    a, b = float(do._coef(s.sqrt_recip_alphas_cumprod, 49)), float(do._coef(s.sqrt_recipm1_alphas_cumprod, 49))
    over = np.abs(x0 - want_x0) - (a * np.abs(sample[-2] - want_sample[-2]) + b * np.abs(sample[-1] - want_sample[-1]) + X0_ROUNDING)
    assert float(over.max()) <= 0.0, float(over.max())


@pytest.mark.parametrize("case", ir.M_CASES)
def test_model_level_restatement_equals_fixture(case):
    z = _golden()
    sample, x0 = pinned(_model_restatement, case)
    _check_chain(sample, x0, z[f"M::{case}::sample"], z[f"M::{case}::pred_xstart"])
    if case == "guided":      # the halves of the doubled batch stay bit-identical (the update reads no variance channel)
        assert np.array_equal(sample[:, :2], sample[:, 2:]) and np.array_equal(x0[:2], x0[2:])


def _kernel_digests(tag):
    return [(ir.kernel_key(tag, clip, spec, shape, index), *ir.kernel_digest(ir.kernel_restatement(tag, clip, spec, shape, index)))
            for spec, shape, index in ir.kernel_grid() for clip in (True, False)]


@pytest.mark.parametrize("tag", sorted(ir.K_TYPES))
def test_kernel_level_restatement_equals_fixture(tag):
    """Equal bits, in the pinned child: torch takes sin / cos of the synthetic model from MKL's vector library, which follows
    MKL_CBWR as the GEMMs do."""
    z = _golden()
    for key, vals, sums in pinned(_kernel_digests, tag):
        assert np.array_equal(vals, z[key]), key
        assert np.allclose(sums, z[key + "::sums"], rtol=1e-12, atol=0.0), key     # fp64 sums of equal fp32 values: the order only


def test_last_index_returns_eps_and_the_next_table_is_shifted():
    """alphas_cumprod_next[T-1] = 0: the step at T-1 returns the re-derived eps itself; elsewhere next[i] = alphas_cumprod[i + 1]."""
    s = do.Schedule("50")
    nxt = ir.alphas_cumprod_next(s)
    assert nxt[-1] == 0.0 and np.array_equal(nxt[:-1], s.alphas_cumprod[1:])
    _, _, x_t, mo = ir.kernel_inputs(s, ir.K_SHAPES[0], 49)
    r = ir.ddim_reverse_sample(s, mo, x_t, 49, False)
    eps = (do._coef(s.sqrt_recip_alphas_cumprod, 49) * x_t - r["pred_xstart"]) / do._coef(s.sqrt_recipm1_alphas_cumprod, 49)
    assert torch.equal(r["sample"], eps)


def _fresh_reference(monkeypatch):
    # the timm stand-in and the reference modules leave sys.modules with the test (other tests probe for the real timm)
    for name in ("timm", "timm.models", "timm.models.vision_transformer", "_reference_latte", "_reference_diffusion"):
        if name not in sys.modules:
            monkeypatch.setitem(sys.modules, name, None)
            del sys.modules[name]


@pytest.mark.skipif(not reference_available(), reason="the reference checkout is present only where the fixture is generated")
@pytest.mark.parametrize("case", ir.M_CASES)
def test_restatement_equals_live_reference(monkeypatch, case):
    """Both sides in this process on one thread and one MKL code path, whichever the host's is."""
    _fresh_reference(monkeypatch)
    want = ir.reference_model_chain(case)
    got = ir.model_restatement(case)
    _check_chain(got["sample"], got["pred_xstart"], want["sample"], want["pred_xstart"])


@pytest.mark.parametrize("spec", SPECS)
def test_alphas_cumprod_next_table(monkeypatch, spec):
    """latte_schedule_table("alphas_cumprod_next") = append(alphas_cumprod[1:], 0.0) (gd:174) of the same schedule, bit for bit; and
    the reference's own table where the reference is present."""
    import latte_amd
    d = latte_amd.create_diffusion(spec)
    n = d.num_timesteps
    assert d.alphas_cumprod_next.shape == (n,) and d.alphas_cumprod_next[-1] == 0.0
    assert np.array_equal(d.alphas_cumprod_next[:-1], d.alphas_cumprod[1:])
    assert np.array_equal(d.alphas_cumprod_next, ir.alphas_cumprod_next(do.Schedule(spec)))
    if reference_available():
        _fresh_reference(monkeypatch)
        from oracle import reference_loader as rl
        assert np.array_equal(d.alphas_cumprod_next, rl.load_reference_diffusion().create_diffusion(spec).alphas_cumprod_next)
