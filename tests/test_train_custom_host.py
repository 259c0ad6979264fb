"""Host side of the custom-loss path, no GPU: the three new C-ABI calls are declared, exported and prototyped alike (as
tests/test_abi.py checks the whole surface), and the training config's ``loss_fn: "package.module:function"`` resolver."""
import ctypes
import os
import re

import pytest

from _util import ROOT

NEW = ("latte_trainer_forward", "latte_trainer_seed", "latte_trainer_input_grad")
NEW_DEBUG = ("latte_debug_patch_embed_dgrad",)

NOT_CALLABLE = 3          # resolver targets in this module: this and the function below


def per_sample_mse(out, x_start, x_t, t, noise):
    return ((noise - out) ** 2).flatten(1).mean(1)


def eps_mse(out, x_start, x_t, t, noise):
    """The MSE on the mean head of a learned-sigma model (what the training driver's test points ``loss_fn:`` at)."""
    return ((noise - out[:, :, :noise.shape[2]]) ** 2).flatten(1).mean(1)


def declaration(name, header):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\b(\w[\w\s\*]*?)\b%s\s*\(([^)]*)\)\s*;" % name, src)
    assert m, f"{name} is not declared in include/{header}"
    return m.group(1).strip(), [a.strip() for a in m.group(2).split(",")]


def ctype_of(param):
    if "*" in param:
        return ctypes.c_void_p
    kind = param.rsplit(None, 1)[0].replace("const", "").strip()
    return {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "double": ctypes.c_double}[kind]


@pytest.mark.parametrize("name,header", [(n, "latte_amd.h") for n in NEW] + [(n, "latte_amd_debug.h") for n in NEW_DEBUG])
def test_prototype_agrees_with_the_header(lib, name, header):
    from latte_amd._lib import PROTOTYPES
    ret, params = declaration(name, header)
    assert ret == "int"
    assert name in PROTOTYPES, name
    restype, argtypes = PROTOTYPES[name]
    assert restype is ctypes.c_int
    assert [ctype_of(p) for p in params] == list(argtypes), (params, argtypes)
    assert hasattr(lib, name), f"{name} is declared but not exported"


def test_new_calls_refuse_null_handles(lib):
    """Argument validation runs before anything touches a device."""
    for name, args in (("latte_trainer_forward", (None, None, None, None, 1, None, None)), ("latte_trainer_seed", (None, None, None)),
                       ("latte_trainer_input_grad", (None, None, None)),
                       ("latte_debug_patch_embed_dgrad", (None, None, None, 1, 1, 2, 4, 128, None, None))):
        assert getattr(lib, name)(*args) != 0, name
        assert lib.latte_last_error()


def test_loss_fn_resolver():
    from latte_amd.train_util import resolve_loss_fn
    assert resolve_loss_fn(None) is None and resolve_loss_fn("") is None
    assert resolve_loss_fn("test_train_custom_host:per_sample_mse") is per_sample_mse
    import torch.nn.functional as F
    assert resolve_loss_fn("torch.nn.functional:mse_loss") is F.mse_loss
    with pytest.raises(ValueError, match="package.module:function"):
        resolve_loss_fn("test_train_custom_host.per_sample_mse")            # the colon is missing
    with pytest.raises(ValueError, match="package.module:function"):
        resolve_loss_fn("test_train_custom_host:")
    with pytest.raises(ValueError, match="no attribute 'nothing_here'"):
        resolve_loss_fn("test_train_custom_host:nothing_here")
    with pytest.raises(ValueError, match="not callable"):
        resolve_loss_fn("test_train_custom_host:NOT_CALLABLE")
    with pytest.raises(ValueError, match="cannot import module"):
        resolve_loss_fn("no_such_package_anywhere.losses:mse")
