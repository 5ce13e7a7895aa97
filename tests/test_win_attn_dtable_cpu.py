"""Host side of the fused relative-position-table gradient (OCPG_WIN_ATTN_FUSED_DTABLE): the C ABI declares and binds the two entry
points, and `table_codes` finds the per-token codes with index[q, k] = code[q] - code[k] + off for the reference's sliced index
(full and clamped windows) -- and refuses an index that is not of that form."""
import os
import re

import pytest
import torch

from conftest import ROOT

SYMBOLS = ("ocpg_win_attn_dtable_supported", "ocpg_win_attn_bwd_mfma_dtable")


def test_header_declares_and_ctypes_binds_the_dtable_entry_points():
    import ctypes
    from ocpg_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ocpg_hip.h")).read(), flags=re.S)
    for s in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % s, src), f"{s} not declared in include/ocpg_hip.h"
        assert s in _lib.SIGNATURES, f"{s} not bound in _lib.SIGNATURES"
    assert _lib.SIGNATURES["ocpg_win_attn_dtable_supported"] == [ctypes.c_int] * 4
    # the arguments of ocpg_win_attn_bwd_mfma up to Dbuf, then tok_code, code_off, T, partials, dtable in place of dS
    old, new = _lib.SIGNATURES["ocpg_win_attn_bwd_mfma"], _lib.SIGNATURES["ocpg_win_attn_bwd_mfma_dtable"]
    assert new[:15] == old[:15] and new[-2:] == old[-2:]
    assert new[15:-2] == [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    # the entry point is documented next to the other window-attention ones
    assert "ocpg_win_attn_bwd_mfma_dtable" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def _index(window):
    import ocpg_amd.models.video_swin_transformer as vs
    return vs.WindowAttention3D(32, window, 1).relative_position_index


@pytest.mark.parametrize("window,n", [((8, 7, 7), 392), ((8, 7, 7), 245), ((8, 7, 7), 37), ((2, 7, 7), 98), ((2, 7, 7), 37)])
def test_table_codes_reproduce_the_sliced_index(window, n):
    from ocpg_amd.models.ops.functions.win_attn_func import table_codes
    full = _index(window)
    idx = full[:n, :n]                                     # the reference's slice: a view with the full row stride
    code, off = table_codes(idx)
    assert code.dtype == torch.int32 and code.shape == (n,) and isinstance(off, int)
    rebuilt = code.long()[:, None] - code.long()[None, :] + off
    assert torch.equal(rebuilt, idx)
    rows = (2 * window[0] - 1) * (2 * window[1] - 1) * (2 * window[2] - 1)
    assert 0 <= int(rebuilt.min()) and int(rebuilt.max()) < rows


def test_table_codes_refuse_a_non_linear_index_and_cache_per_n_and_device():
    from ocpg_amd.models.ops.functions.win_attn_func import table_codes
    full = _index((8, 7, 7))
    for q, k in ((5, 9), (0, 0), (36, 0), (0, 36)):
        bad = full[:37, :37].clone()
        bad[q, k] += 1
        assert table_codes(bad) is None, (q, k)
    assert table_codes(full[:37, :36]) is None             # not square
    cache = {}
    first = table_codes(full[:245, :245], cache)
    assert table_codes(full[:245, :245], cache) is first and list(cache) == [(245, full.device)]
    other = table_codes(full[:37, :37], cache)
    assert other is not first and other[0].shape == (37,) and len(cache) == 2
    bad = full[:98, :98].clone()
    bad[3, 4] -= 1
    assert table_codes(bad, cache) is None and cache[(98, full.device)] is None       # the refusal is remembered too
