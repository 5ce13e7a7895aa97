"""Fused front end of the 16-bit MSDeformAttn value path (ocpg_msda_fused_fwd_h16 / ocpg_msda_fused_bwd_qproj_h16, OCPG_MSDA_FUSED_FRONT_H16):
what can be checked without a GPU -- the C-ABI boundary and the default of the switch."""
import ctypes
import os
import subprocess
import sys

from test_abi import declared_symbols

FUSED_H16_SYMBOLS = ("ocpg_msda_fused_fwd_h16", "ocpg_msda_fused_bwd_qproj_h16")


def test_header_library_and_ctypes_table_agree_on_the_fused_h16_symbols():
    from ocpg_amd import _lib
    from ocpg_amd.csrc import build
    build.build()
    syms = declared_symbols()
    L = ctypes.CDLL(_lib.LIB_PATH)
    for s in FUSED_H16_SYMBOLS:
        assert s in syms, f"{s} not declared in include/ocpg_hip.h"
        assert hasattr(L, s), f"{s} not exported by libocpg_hip.so"
        assert s in _lib.SIGNATURES, f"{s} not bound in _lib.SIGNATURES"
    # trailing `int dtype` before `stream`; the fp32 symbols' argument lists with that one int added
    for s in FUSED_H16_SYMBOLS:
        f32 = _lib.SIGNATURES[s.replace("_h16", "_f32")]
        assert _lib.SIGNATURES[s] == f32[:-1] + [ctypes.c_int, ctypes.c_void_p], s
    header = open(os.path.join(os.path.dirname(_lib._HERE), "include", "ocpg_hip.h")).read()
    assert "has no 16-bit form" not in header


def test_switch_is_off_when_the_variable_is_unset():
    """(read once at import: a fresh interpreter without the variable, then with "0" and "1")"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = "from ocpg_amd.models.ops.modules import ms_deform_attn as m; print(int(m.FUSED_FRONT_H16))"
    for word, want in ((None, "0"), ("0", "0"), ("1", "1")):
        env = {k: v for k, v in os.environ.items() if k != "OCPG_MSDA_FUSED_FRONT_H16"}
        if word is not None:
            env["OCPG_MSDA_FUSED_FRONT_H16"] = word
        out = subprocess.run([sys.executable, "-c", code], cwd=root, env=env, capture_output=True, text=True, check=True).stdout.split()
        assert out[-1] == want, (word, out)
