"""ocpg_amd/_lib.py binds the C ABI from include/*.h: the parser on a synthetic header, its refusals, a spot check of the real header
against hand-written signatures, and the set of entry points that launch nothing.  No GPU and no library needed."""
import ctypes
import glob
import os
import re

import pytest

from ocpg_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_vp = ctypes.c_void_p
_int = ctypes.c_int
_ll = ctypes.c_longlong
_ull = ctypes.c_ulonglong
_f = ctypes.c_float
_d = ctypes.c_double

SYNTHETIC = """/* a header in the style of include/ocpg_hip.h
 * int fake_in_a_comment(int a, void* stream);
 */
#ifndef SYNTHETIC_H
#define SYNTHETIC_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
int all_pointers(const float* a, void* b, const void* const* c, const int64_t* d, const unsigned char* e, void* stream);
int all_scalars(int a, long long b, unsigned long long c, float d, double e);
long long no_parameters(void);
long long empty_list();
/* void another_fake(double x); */
int over_four_lines(const float* x, long long rows,
                    int cols,   /* int not_a_parameter, */
                    float eps, unsigned long long seed,
                    float *y, void* stream);
void returns_nothing(int on);
const char* returns_text(void);
const char *returns_text_too(void);
#ifdef __cplusplus
}
#endif
#endif
"""


def test_parser_on_a_synthetic_header():
    assert _lib.parse_header(SYNTHETIC) == {
        "all_pointers": (_int, [_vp] * 6),
        "all_scalars": (_int, [_int, _ll, _ull, _f, _d]),
        "no_parameters": (_ll, []),
        "empty_list": (_ll, []),
        "over_four_lines": (_int, [_vp, _ll, _int, _f, _ull, _vp, _vp]),
        "returns_nothing": (None, [_int]),
        "returns_text": (ctypes.c_char_p, []),
        "returns_text_too": (ctypes.c_char_p, []),
    }


@pytest.mark.parametrize("decl, names", [
    ("int takes_a_short(const float* x, short n, void* stream);", ("takes_a_short", "'n'", "short")),
    ("int takes_unsigned(unsigned int n);", ("takes_unsigned", "'n'", "unsigned int")),
    ("int takes_a_struct(dim3 grid, void* stream);", ("takes_a_struct", "'grid'", "dim3")),
    ("float returns_float(int n);", ("returns_float", "float")),
    ("unsigned long long returns_u64(void);", ("returns_u64", "unsigned long long")),
    ("void* returns_pointer(int n);", ("returns_pointer", "void*")),
], ids=["short", "unsigned", "struct", "ret-float", "ret-u64", "ret-pointer"])
def test_unknown_types_raise_and_name_the_symbol(decl, names):
    with pytest.raises(ValueError) as e:
        _lib.parse_header("int fine(int n);\n" + decl)
    for n in names:
        assert n in str(e.value)


def test_what_is_not_a_plain_declaration_raises():
    with pytest.raises(ValueError):
        _lib.parse_header("int f(int n);  // a line comment\n")
    with pytest.raises(ValueError):
        _lib.parse_header("int takes_a_callback(void (*cb)(int), void* stream);")
    with pytest.raises(ValueError):
        _lib.parse_header("typedef int ocpg_status;")


# copied verbatim from the hand-written table this parser replaced: symbols where one wrong scalar width shifts every later argument
HAND_WRITTEN = {
    "ocpg_bn_act_fwd": [_vp, _vp, _vp, _vp, _vp, ctypes.c_longlong, _int, ctypes.c_longlong, _int, _int, _vp],
    "ocpg_gemm": [_vp, _vp, _vp, _vp] + [_int] * 4 + [ctypes.c_longlong] * 10 + [ctypes.c_float, ctypes.c_float, _vp],
    "ocpg_gemm_set_tuning": [_int],
    "ocpg_gemm_export_picks": [_vp, ctypes.c_longlong],
    "ocpg_groupnorm_cl_fwd": [_vp, _int, _vp, _vp, ctypes.c_longlong, _int, _int, _int, ctypes.c_float, _vp, _vp, _vp, _vp, _vp],
    "ocpg_matcher_cost_f32": [_vp] * 3 + [ctypes.c_longlong] * 4 + [_vp] * 4 + [_int] * 7 + [ctypes.c_float] * 5 + [_vp] * 4,
    "ocpg_dropout_add_ln_fwd_ex": [_vp] * 4 + [ctypes.c_longlong, _int, ctypes.c_float, ctypes.c_float, ctypes.c_ulonglong, ctypes.c_ulonglong, _vp, _int]
                                  + [_vp] * 6 + [_int, _vp],
    "ocpg_adamw_step": [_vp] * 8 + [_int, ctypes.c_longlong, _vp, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_longlong, _vp],
    "ocpg_grad_norm_clip_amp": [_vp] * 3 + [_int, ctypes.c_longlong, ctypes.c_float, _vp, _vp, _vp, ctypes.c_double, ctypes.c_double, _vp, _vp],
    "ocpg_lfm_spectrum_inv": [_vp, _int, _vp, _vp, _vp, _vp] + [_int] * 4 + [_vp, _vp, ctypes.c_float, _vp, _vp, _vp, _vp],
    "ocpg_attn_longk_bwd": [_vp, ctypes.c_longlong, _vp, ctypes.c_longlong, _vp, ctypes.c_longlong, _vp, _vp, ctypes.c_longlong, _vp,
                            ctypes.c_longlong, _vp, ctypes.c_float] + [_int] * 5 + [ctypes.c_float, ctypes.c_ulonglong, ctypes.c_ulonglong, _vp,
                                                                                    _vp, ctypes.c_longlong, _vp, _vp, _int, _vp],
    "ocpg_mask_tail_f32": [_vp] + [_int] * 10 + [ctypes.c_float, ctypes.c_float, _int, _vp, _vp],
    "ocpg_clip_front_u8": [_vp, _int, ctypes.c_longlong, ctypes.c_longlong] + [_int] * 6 + [_vp, _vp, _int, _vp, _vp, _int] + [_int] * 6
                          + [_vp, ctypes.c_longlong, ctypes.c_longlong, _vp, _vp],
    "ocpg_memfuse_fwd_f32": [_vp] * 4 + [ctypes.c_longlong] * 2 + [_int] * 5 + [_vp] * 3,
}
LONG_LONG_RETURNS = ("ocpg_gemm_plans", "ocpg_gemm_tuned", "ocpg_gemm_tune_rejected", "ocpg_gemm_export_picks",
                     "ocpg_bias_relu_dropout_bwd_slots", "ocpg_dropout_add_ln_bwd_slots", "ocpg_groupnorm_cl_work", "ocpg_colsum_blocks",
                     "ocpg_sim_heat_workspace", "ocpg_target_pack_workspace")


def _header_text():
    return "".join(open(h).read() for h in sorted(glob.glob(os.path.join(ROOT, "include", "*.h"))))


def test_real_header_against_hand_written_signatures():
    parsed = _lib.parse_header(_header_text())
    for name, argtypes in HAND_WRITTEN.items():
        assert parsed[name][1] == argtypes, name
        assert _lib.SIGNATURES[name] == argtypes, name
    assert {name for name, (restype, _) in parsed.items() if restype is ctypes.c_longlong} == set(LONG_LONG_RETURNS)
    assert [name for name, (restype, _) in parsed.items() if restype is None] == ["ocpg_gemm_set_tuning"]
    assert [name for name, (restype, _) in parsed.items() if restype is ctypes.c_char_p] == ["ocpg_hip_version"]
    assert all(parsed[name][0] is _int for name in HAND_WRITTEN if name not in LONG_LONG_RETURNS + ("ocpg_gemm_set_tuning",))
    # what lib() binds is this parse, and SIGNATURES is its argument lists without the version string
    assert {name: argtypes for name, (_, argtypes) in parsed.items() if name != "ocpg_hip_version"} == _lib.SIGNATURES


# the hand-kept tuple the rule replaced, and the five host-side entry points it had missed
WAS_UNTIMED = ("ocpg_lsfeat_bwd_parts", "ocpg_sim_heat_workspace", "ocpg_text_gate_rows", "ocpg_text_gate_splits", "ocpg_win_attn_dtable_supported", "ocpg_conv3x3_mfma_body_splits", "ocpg_gemm_dgrad_bn_tile", "ocpg_conv3x3_mfma_wgrad_splits", "ocpg_window_sums3x3_cl_bands", "ocpg_lfm_dft_supported", "ocpg_lfm_dft_split", "ocpg_conv3x3_mfma_splits", "ocpg_gemm_set_tuning", "ocpg_gemm_export_picks", "ocpg_gemm_import_picks", "ocpg_colsum_blocks", "ocpg_mso_wgrad_rows", "ocpg_gemm_plans", "ocpg_gemm_tuned", "ocpg_gemm_tune_rejected", "ocpg_bias_relu_dropout_bwd_slots", "ocpg_dropout_add_ln_bwd_slots", "ocpg_groupnorm_cl_work")
NOW_ALSO = ("ocpg_layernorm_blocks", "ocpg_target_pack_workspace", "ocpg_graph_replace_memsets", "ocpg_graph_stats", "ocpg_graph_memcpy_nodes")


def test_entry_points_that_launch_nothing():
    assert len(set(WAS_UNTIMED)) == 23 and not set(WAS_UNTIMED) & set(NOW_ALSO)
    assert set(_lib._UNTIMED) == set(WAS_UNTIMED) | set(NOW_ALSO)
    # an independent reading of the header: the parameter list of every declaration, comments removed
    text = re.sub(r"/\*.*?\*/", "", _header_text(), flags=re.S)
    params = dict(re.findall(r"\b(ocpg_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text))
    assert set(params) == set(_lib.SIGNATURES) | {"ocpg_hip_version"}
    for name in _lib.SIGNATURES:
        assert (name in _lib._UNTIMED) == (re.search(r"\bstream\b", params[name]) is None), name
    # the proxy hands these out raw: no census count, no event pair
    raw = object()
    proxy = _lib._Lib(type("FakeCDLL", (), {"__getattr__": lambda self, name: raw})())
    assert all(getattr(proxy, name) is raw for name in _lib._UNTIMED)
    assert proxy.ocpg_layernorm_fwd is not raw and proxy.ocpg_msda_fwd_f32 is not raw
