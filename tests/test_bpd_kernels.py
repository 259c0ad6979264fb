"""The likelihood kernels one call at a time: latte_bpd_terms (one column of calc_bpd_loop, gaussian_diffusion.py:839-852) and
latte_prior_bpd (:797-811) against tests/golden/bpd.npz -- what the reference computed on the kernel-level fixtures of
tests/bpd_reference.py: every ModelMeanType x ModelVarType, clip_denoised on and off, 432 / 1024 / 65 536 elements per sample
(ragged, one block, many blocks), the first, second, middle and last index.

Bound: 2e-5 entry-wise relative, the bound tests/test_training_losses.py holds the sibling terms kernel to -- the same fp32
operation sequence on the same inputs; expf / logf / tanhf are the device's and the mean is taken in another order."""
import ctypes
import os

import numpy as np
import pytest
import torch

import bpd_reference as br
from _util import GOLDEN, rel_l2
from oracle import diffusion_oracle as do

pytestmark = pytest.mark.gpu
TOL = 2e-5


def _golden():
    return np.load(os.path.join(GOLDEN, "bpd.npz"))


_record, _rel = br.record, br.rel_max


def _terms(d, case, index, clip, want_xstart=False):
    """latte_bpd_terms through the shim on device copies of a case's (x0, noise, x_t, model_out) -> [3, B] on the host, pred_xstart."""
    x0, nz, x_t, mo = (v.cuda() for v in case)
    tables, pred = d._bpd_terms(x0, x_t, nz, mo, index, clip, want_xstart=want_xstart)
    return torch.stack([t[:, 0] for t in tables]).cpu(), pred


@pytest.mark.parametrize("clip", [True, False], ids=["clip", "noclip"])
@pytest.mark.parametrize("tag", sorted(br.K_TYPES))
def test_bpd_terms_match_reference(tag, clip):
    import latte_amd
    z = _golden()
    worst = [0.0, 0.0, 0.0]
    worst_x0 = 0.0
    for spec, shape, index in br.kernel_grid():
        kw = br.K_TYPES[tag]
        d = latte_amd.create_diffusion(spec, **kw)
        s = do.Schedule(spec, **kw)
        case = br.kernel_inputs(s, shape, index)
        got, pred = _terms(d, case, index, clip, want_xstart=True)
        want = z[br.kernel_key(tag, clip, spec, shape, index)]
        assert torch.isfinite(got).all()
        err = [_rel(got[j].numpy(), want[j]) for j in range(3)]
        print(tag, clip, spec, shape, index, err)
        worst = [max(a, b) for a, b in zip(worst, err)]
        want_x0 = br.bpd_terms(s, case[3], case[0], case[2], case[1], index, clip)[3]
        worst_x0 = max(worst_x0, rel_l2(pred, want_x0))
        assert max(err) < TOL, (tag, clip, spec, shape, index, err, got, want)
        assert rel_l2(pred, want_x0) < 1e-6
    _record(f"kernel::{tag}::clip{int(clip)}", {"vb": worst[0], "xstart_mse": worst[1], "mse": worst[2], "pred_xstart_rel_l2": worst_x0})


def test_prior_bpd_matches_reference():
    import latte_amd
    z = _golden()
    worst = 0.0
    for spec, shape in [("50", sh) for sh in br.K_SHAPES] + [("", br.K_SHAPES[0])]:
        d = latte_amd.create_diffusion(spec)
        x0, _ = br.kernel_x_start(shape)
        got = d._prior_bpd(x0.cuda()).cpu().numpy()
        err = _rel(got, z[f"K::prior::{spec or 'full'}::{shape[0]}x{shape[1]}"])
        print(spec, shape, err)
        worst = max(worst, err)
        assert err < TOL, (spec, shape, got)
    _record("kernel::prior_bpd", worst)


def test_two_runs_give_equal_bits_and_rows_do_not_depend_on_the_batch():
    import latte_amd
    d = latte_amd.create_diffusion("50")
    s = do.Schedule("50")
    for shape in (br.K_SHAPES[0], br.K_SHAPES[2]):
        for index in (0, 25):
            case = br.kernel_inputs(s, shape, index)
            a, pa = _terms(d, case, index, True, want_xstart=True)
            b, pb = _terms(d, case, index, True, want_xstart=True)
            assert torch.equal(a, b) and torch.equal(pa, pb)
            one, _ = _terms(d, tuple(v[:1].contiguous() for v in case), index, True)      # sample 0 alone, B = 1
            assert torch.equal(one[:, 0], a[:, 0]), (shape, index, one[:, 0], a[:, 0])
        x0 = case[0].cuda()
        p = d._prior_bpd(x0)
        assert torch.equal(p, d._prior_bpd(x0)) and torch.equal(p[:1], d._prior_bpd(x0[:1].contiguous()))


def _raw_call(lib, d, case, index, tables, column, stride, override=None):
    from latte_amd._lib import ptr, stream_ptr
    x0, nz, x_t, mo = case
    B, F, C = x0.shape[:3]
    hw = x0.shape[3] * x0.shape[4]
    need = int(lib.latte_bpd_workspace_floats(B, x0[0].numel()))
    ws = torch.empty(need, device="cuda")
    a = dict(s=d._h, index=index, clip=1, x0=ptr(x0), xt=ptr(x_t), nz=ptr(nz), mo=ptr(mo), ws=ptr(ws), nws=need,
             vb=ptr(tables[0][:, column:]), xm=ptr(tables[1][:, column:]), ms=ptr(tables[2][:, column:]))
    a.update(override or {})
    return lib.latte_bpd_terms(a["s"], a["index"], a["clip"], a["x0"], a["xt"], a["nz"], a["mo"], B, F, C, hw, a["ws"], a["nws"], a["vb"],
                               a["xm"], a["ms"], stride, None, stream_ptr())


def test_out_stride_leaves_neighbouring_columns_untouched(lib):
    import latte_amd
    d = latte_amd.create_diffusion("50")
    case = tuple(v.cuda() for v in br.kernel_inputs(do.Schedule("50"), br.K_SHAPES[0], 25))
    tables = tuple(torch.full((3, 5), -7.0 - j, device="cuda") for j in range(3))
    assert _raw_call(lib, d, case, 25, tables, 2, 5) == 0, lib.latte_last_error()
    torch.cuda.synchronize()
    alone, _ = _terms(d, case, 25, True)
    for j in range(3):
        t = tables[j].cpu()
        assert torch.equal(t[:, 2], alone[j])
        assert bool((t[:, [0, 1, 3, 4]] == -7.0 - j).all())


def test_bad_arguments_are_refused_without_a_launch(lib):
    import latte_amd
    from latte_amd._lib import ptr, stream_ptr
    d = latte_amd.create_diffusion("50")
    case = tuple(v.cuda() for v in br.kernel_inputs(do.Schedule("50"), br.K_SHAPES[0], 25))
    tables = tuple(torch.full((3, 1), -3.0, device="cuda") for _ in range(3))
    null = ctypes.c_void_p(None)
    INVALID = 1
    for override, word in ((dict(x0=null), b"null"), (dict(mo=null), b"null"), (dict(nz=null), b"null"), (dict(ws=null), b"null"),
                           (dict(vb=null), b"null"), (dict(s=null), b"null"), (dict(index=50), b"index"), (dict(index=-1), b"index"),
                           (dict(nws=8), b"workspace")):
        rc = _raw_call(lib, d, case, 25, tables, 0, 1, override)
        assert rc == INVALID and word in lib.latte_last_error(), (override, rc, lib.latte_last_error())
    out = torch.full((3,), -3.0, device="cuda")
    assert lib.latte_prior_bpd(d._h, None, 3, 432, ptr(out), stream_ptr()) == INVALID and b"null" in lib.latte_last_error()
    assert lib.latte_prior_bpd(d._h, ptr(case[0]), 3, 432, None, stream_ptr()) == INVALID
    assert lib.latte_prior_bpd(d._h, ptr(case[0]), 0, 432, ptr(out), stream_ptr()) == INVALID
    torch.cuda.synchronize()
    assert bool((out == -3.0).all()) and all(bool((t == -3.0).all()) for t in tables)      # nothing was launched
