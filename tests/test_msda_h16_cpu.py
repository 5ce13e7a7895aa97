"""16-bit-storage MSDeformAttn (ocpg_msda_*_h16, MSDeformAttn(value_dtype=...), args.msda_value_dtype): what can be checked without a
GPU -- the C-ABI boundary, the public switch and its resolution order, and the error contract of the op for CPU tensors."""
import ctypes

import pytest
import torch

import cases
from test_abi import declared_symbols

H16_SYMBOLS = ("ocpg_msda_fwd_h16", "ocpg_msda_bwd_h16", "ocpg_msda_bwd_value_h16", "ocpg_msda_bwd_locattn_h16")


def test_header_library_and_ctypes_table_agree_on_the_h16_symbols():
    from ocpg_amd import _lib
    from ocpg_amd.csrc import build
    build.build()
    syms = declared_symbols()
    L = ctypes.CDLL(_lib.LIB_PATH)
    for s in H16_SYMBOLS:
        assert s in syms, f"{s} not declared in include/ocpg_hip.h"
        assert hasattr(L, s), f"{s} not exported by libocpg_hip.so"
        assert s in _lib.SIGNATURES, f"{s} not bound in _lib.SIGNATURES"
    # trailing `int dtype` before `stream`, void* 16-bit buffers
    assert _lib.SIGNATURES["ocpg_msda_fwd_h16"][-2:] == [ctypes.c_int, ctypes.c_void_p]
    assert _lib.SIGNATURES["ocpg_msda_bwd_h16"][-2:] == [ctypes.c_int, ctypes.c_void_p]


def _msda_modules(model):
    from ocpg_amd.models.ops.modules import MSDeformAttn
    return [m for m in model.modules() if isinstance(m, MSDeformAttn)]


def _build(monkeypatch, env=None, **over):
    from ocpg_amd.models import build_model
    if env is None:
        monkeypatch.delenv("OCPG_MSDA_VALUE_DTYPE", raising=False)
    else:
        monkeypatch.setenv("OCPG_MSDA_VALUE_DTYPE", env)
    torch.manual_seed(0)
    return build_model(cases.default_args(device="cpu", **cases.TINY, **over))[0]


def test_default_build_keeps_the_fp32_island(monkeypatch):
    from ocpg_amd.models import build_model
    assert cases.default_args().msda_value_dtype is None
    monkeypatch.delenv("OCPG_MSDA_VALUE_DTYPE", raising=False)
    torch.manual_seed(0)
    model = build_model(cases.default_args(device="cpu"))[0]          # default depth: 4 encoder + 4 decoder layers
    mods = _msda_modules(model)
    assert len(mods) == 8
    assert all(m.value_dtype is None for m in mods)


def test_switch_sets_every_module_and_keeps_the_state_dict(monkeypatch):
    from ocpg_amd.models import build_model
    monkeypatch.delenv("OCPG_MSDA_VALUE_DTYPE", raising=False)
    torch.manual_seed(0)
    base = build_model(cases.default_args(device="cpu"))[0]
    torch.manual_seed(0)
    m16 = build_model(cases.default_args(device="cpu", msda_value_dtype="bf16"))[0]
    mods = _msda_modules(m16)
    assert len(mods) == 8 and all(m.value_dtype == torch.bfloat16 for m in mods)
    assert list(base.state_dict().keys()) == list(m16.state_dict().keys())
    m16.load_state_dict(base.state_dict())                      # checkpoints load either way
    base.load_state_dict(m16.state_dict())
    tiny = _build(monkeypatch, msda_value_dtype="fp16")
    assert all(m.value_dtype == torch.float16 for m in _msda_modules(tiny))
    tiny = _build(monkeypatch, msda_value_dtype="autocast")
    assert all(m.value_dtype == "autocast" for m in _msda_modules(tiny))


def test_environment_variable_only_when_the_field_is_none(monkeypatch):
    assert all(m.value_dtype == torch.bfloat16 for m in _msda_modules(_build(monkeypatch, env="bf16")))
    assert all(m.value_dtype == torch.float16 for m in _msda_modules(_build(monkeypatch, env="fp16")))
    assert all(m.value_dtype is None for m in _msda_modules(_build(monkeypatch, env="bf16", msda_value_dtype="fp32")))   # explicit fp32 beats it
    assert all(m.value_dtype == torch.float16 for m in _msda_modules(_build(monkeypatch, env="bf16", msda_value_dtype="fp16")))
    assert all(m.value_dtype is None for m in _msda_modules(_build(monkeypatch, env="fp32")))


def test_reference_side_namespace_without_the_field(monkeypatch):
    from ocpg_amd.models.deformable_transformer import build_deforamble_transformer
    monkeypatch.delenv("OCPG_MSDA_VALUE_DTYPE", raising=False)
    args = cases.default_args(device="cpu", **cases.TINY)
    del args.msda_value_dtype
    tr = build_deforamble_transformer(args)
    assert all(m.value_dtype is None for m in _msda_modules(tr))


@pytest.mark.parametrize("where", ["field", "env"])
def test_unknown_word_raises_at_build_time(monkeypatch, where):
    with pytest.raises(ValueError, match="bf16"):
        if where == "field":
            _build(monkeypatch, msda_value_dtype="fp8")
        else:
            _build(monkeypatch, env="half")


def test_value_dtype_is_inert_on_cpu_inputs(monkeypatch):
    """16-bit mode is a GPU mode: on CPU tensors the module keeps the fp32 path (host-logic tests run the op's test double there)."""
    from ocpg_amd.models.ops.modules import MSDeformAttn
    m = MSDeformAttn(32, 2, 2, 2, value_dtype=torch.bfloat16)
    assert m.active_value_dtype(torch.zeros(1, 4, 32)) is None
    with pytest.raises(ValueError):
        MSDeformAttn(32, 2, 2, 2, value_dtype=torch.float64)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_sixteen_bit_cpu_value_raises_the_gpu_error_not_the_dtype_error(dtype):
    from ocpg_amd.models.ops.functions import MSDeformAttnFunction
    v = torch.zeros(1, 4, 1, 4, dtype=dtype)
    shapes = torch.tensor([[2, 2]])
    ls = torch.tensor([0])
    loc = torch.zeros(1, 1, 1, 1, 1, 2)
    attn = torch.ones(1, 1, 1, 1, 1)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        MSDeformAttnFunction.apply(v, shapes, ls, loc, attn, 64)
