"""fp16 ResNet body, the parts that need no GPU: the three _h16 conv3x3 entry points are declared in the public header and bound in
_lib.SIGNATURES with `int dtype` in front of `stream`, and the Python dtype maps carry fp16 as code 2 (the numbering of ocpg_bn_act_*)."""
import ctypes
import os
import re

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H16_SYMBOLS = {"ocpg_conv3x3_mfma_fwd_cols_h16": "ocpg_conv3x3_mfma_fwd_cols", "ocpg_conv3x3_mfma_dgrad_w_h16": "ocpg_conv3x3_mfma_dgrad_w",
               "ocpg_conv3x3_mfma_wgrad_h16": "ocpg_conv3x3_mfma_wgrad"}


def _header_params(name):
    text = open(os.path.join(ROOT, "include", "ocpg_hip.h")).read()
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{name} is not declared in include/ocpg_hip.h"
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def test_h16_symbols_are_declared_and_bound():
    from ocpg_amd import _lib
    for name, twin in H16_SYMBOLS.items():
        params, old = _header_params(name), _header_params(twin)
        assert params[-1] == "void* stream" and params[-2] == "int dtype", params
        assert params[:-2] == old[:-1], (params, old)              # argument order of the bf16 twin, dtype in front of stream
        sig, old_sig = _lib.SIGNATURES[name], _lib.SIGNATURES[twin]
        assert len(sig) == len(params) == len(old_sig) + 1
        assert sig[:-2] == old_sig[:-1] and sig[-2] is ctypes.c_int and sig[-1] is ctypes.c_void_p


def test_python_dtype_codes():
    from ocpg_amd import _lib
    from ocpg_amd.models.ops.functions import bn_act_func, conv_bn_func
    table = _lib.DTYPE_CODE
    assert table[torch.float32] == 0 and table[torch.bfloat16] == 1 and table[torch.float16] == 2 and len(table) == 3
    assert bn_act_func._DT is table and conv_bn_func._DT is table          # the bindings use that very table, not a copy
    assert not hasattr(conv_bn_func, "_DT3")


def test_fp16_is_not_eligible_where_a_switch_selects_a_bf16_only_kernel(monkeypatch):
    """OCPG_DGRAD_OWN_WEIGHT=0 and OCPG_CONV3X3_SPLITK select kernels without an fp16 form: eligible3x3_mfma sends an fp16 map to the
    library path (bn(conv(x))) before looking at anything else.  (That a bf16 map stays eligible under the switches is a GPU test:
    tests/test_resnet_fp16_gpu.py::test_bf16_map_stays_eligible_under_the_bf16_only_switches.)"""
    from ocpg_amd.models.ops.functions import conv_bn_func as f

    class Map:                      # what eligible3x3_mfma reads of a tensor before its first GPU-only test
        def __init__(self, dtype):
            self.dtype, self.is_cuda = dtype, False

    monkeypatch.setattr(f, "DGRAD_OWN_WEIGHT", False)
    assert f.eligible3x3_mfma(Map(torch.float16), None) is False
    monkeypatch.setattr(f, "DGRAD_OWN_WEIGHT", True)
    monkeypatch.setattr(f, "BODY_SPLITK", True)
    assert f.eligible3x3_mfma(Map(torch.float16), None) is False
