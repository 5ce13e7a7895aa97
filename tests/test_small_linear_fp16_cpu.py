"""The argument contract of the three _h16 entry points of the fp16 decoder / head / neck side (ocpg_small_linear_fwd_h16, ocpg_small_linear_bwd_h16,
ocpg_conv3x3_mfma_fwd_splitk_h16): every refusal below returns before any HIP call, so it is checked here with null / dummy pointers.
dtype 1 = bf16, 2 = fp16, anything else -1010 before any other check; every other check and code is the un-suffixed twin's."""
import ctypes

import pytest

DUMMY = ctypes.c_void_p(64)          # never dereferenced: every call below returns from its argument checks


def _L():
    from ocpg_amd import _lib
    return _lib.lib()


def _fwd(L, r, cin, cout, dtype, x=None, w=None, y=None):
    return L.ocpg_small_linear_fwd_h16(x, 1, w, None, r, cin, cout, 0, y, dtype, None)


def _bwd(L, r, cin, cout, dtype, gy=None):
    return L.ocpg_small_linear_bwd_h16(gy, 1, None, 1, None, None, r, cin, cout, None, None, None, dtype, None)


def _splitk(L, n, cin, dtype, out_dt, splits=2):
    return L.ocpg_conv3x3_mfma_fwd_splitk_h16(None, None, None, n, 5, 5, cin, 64, 2, splits, None, None, out_dt, None, dtype, None)


@pytest.mark.parametrize("bad", [0, 3])
def test_bad_dtype_codes_return_1010_before_any_other_check(bad):
    L = _L()
    # arguments that every OTHER check would refuse too (Cin = 0: -1005 / -1006; Cin = 96: -2000): -1010 comes first
    for cin in (256, 0, 96):
        assert _fwd(L, 50, cin, 256, bad) == -1010
        assert _bwd(L, 50, cin, 256, bad) == -1010
        assert _splitk(L, 1, cin, bad, 0) == -1010
    assert _fwd(L, 50, 256, 256, bad, DUMMY, DUMMY, DUMMY) == -1010
    assert _splitk(L, 1, 256, bad, bad) == -1010


def test_fp16_codes_keep_the_twins_limits_and_return_codes():
    L = _L()
    assert _fwd(L, 50, 96, 256, 2) == -2000 and _bwd(L, 50, 96, 256, 2) == -2000              # Cin not a multiple of 64
    assert _fwd(L, 4097, 256, 256, 2) == -2000 and _bwd(L, 4097, 256, 256, 2) == -2000        # more rows than the kernels serve
    assert _fwd(L, 0, 256, 256, 2) == 0                                                        # nothing to do, nothing launched
    assert _fwd(L, 50, 0, 256, 2) == -1005 and _bwd(L, 50, 0, 256, 2) == -1006
    assert _fwd(L, -1, 256, 256, 2) == -1005 and _bwd(L, -1, 256, 256, 2) == -1006
    # the null-pointer codes of the twins, in their order
    assert _fwd(L, 50, 256, 256, 2) == -1001 and _fwd(L, 50, 256, 256, 2, x=DUMMY) == -1003
    assert _fwd(L, 50, 256, 256, 2, x=DUMMY, w=DUMMY) == -1008
    assert _bwd(L, 50, 256, 256, 2) == -1001 and _bwd(L, 50, 256, 256, 2, gy=DUMMY) == -1003
    assert _bwd(L, 0, 256, 256, 2) == -1001                   # the backward has no R == 0 shortcut (gw = 0 is still written): the twin's code
    # the same arguments give the same codes through dtype 1 and through the un-suffixed symbols
    for r, cin in ((50, 96), (4097, 256), (0, 256), (50, 0), (50, 256)):
        a = L.ocpg_small_linear_fwd(None, 1, None, None, r, cin, 256, 0, None, None)
        assert _fwd(L, r, cin, 256, 1) == a == _fwd(L, r, cin, 256, 2), (r, cin)
        b = L.ocpg_small_linear_bwd(None, 1, None, 1, None, None, r, cin, 256, None, None, None, None)
        assert _bwd(L, r, cin, 256, 1) == b == _bwd(L, r, cin, 256, 2), (r, cin)


def test_splitk_h16_out_dt_is_fp32_or_the_storage_type():
    L = _L()
    assert _splitk(L, 1, 256, 2, 1) == -2000 and _splitk(L, 1, 256, 1, 2) == -2000            # out_dt is 0 or equal to dtype
    assert _splitk(L, 1, 256, 2, 3) == -2000
    for dtype in (1, 2):
        for out_dt in (0, dtype):
            assert _splitk(L, 1, 256, dtype, out_dt) == -1001                                  # accepted: the next check is the null x
            assert _splitk(L, 0, 256, dtype, out_dt) == 0                                      # no images: nothing launched
    assert _splitk(L, 1, 96, 2, 2) == -2000 and _splitk(L, 1, 0, 2, 2) == -1006
    assert _splitk(L, 1, 256, 2, 2, splits=3) == -2000                                         # 4 chunks do not split three ways
    # the un-suffixed symbol forwards with dtype 1: same codes
    un = lambda n, cin, out_dt: L.ocpg_conv3x3_mfma_fwd_splitk(None, None, None, n, 5, 5, cin, 64, 2, 2, None, None, out_dt, None, None)      # noqa: E731
    assert un(1, 256, 2) == -2000 and un(1, 256, 1) == -1001 and un(1, 256, 0) == -1001 and un(0, 256, 1) == 0 and un(1, 0, 1) == -1006
