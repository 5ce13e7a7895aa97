"""C-ABI checks of csrc/attn_longk.hip that need no GPU: the entry points exist, and their shape checks answer before any HIP call
(null pointers, no device)."""
import pytest


@pytest.fixture(scope="module")
def L():
    from ocpg_amd import _lib
    from ocpg_amd.csrc import build
    build.build()
    return _lib.lib()


def _fwd(L, Lq, B, H, hd, Lk):
    #        q     ldq k     ldk v     ldv pad   scale                   pdrop seed offs base out   ldo lse   dtype stream
    return L.ocpg_attn_longk_fwd(None, 0, None, 0, None, 0, None, 1.0, Lq, B, H, hd, Lk, 0.0, 0, 0, None, None, 0, None, 0, None)


def _bwd(L, Lq, B, H, hd, Lk):
    return L.ocpg_attn_longk_bwd(None, 0, None, 0, None, 0, None, None, 0, None, 0, None, 1.0, Lq, B, H, hd, Lk, 0.0, 0, 0, None, None, 0, None,
                                 None, 0, None)


def test_entry_points_exist(L):
    from ocpg_amd import _lib
    assert "ocpg_attn_longk_fwd" in _lib.SIGNATURES and "ocpg_attn_longk_bwd" in _lib.SIGNATURES
    assert callable(L.ocpg_attn_longk_fwd) and callable(L.ocpg_attn_longk_bwd)


@pytest.mark.parametrize("call", [_fwd, _bwd], ids=["fwd", "bwd"])
def test_shape_checks_precede_every_hip_call(L, call):
    assert call(L, 64, 2, 8, 32, 129) == -2000          # more keys than served
    assert call(L, 64, 2, 8, 16, 40) == -2000           # head_dim != 32
    assert call(L, 64, 2, 16, 32, 40) == -2000          # H > 8
    assert call(L, 64, 2, 3, 32, 40) == -2000           # 256 % H != 0
    assert call(L, 64, 65536, 8, 32, 40) == -2000       # B past the grid's y range
    assert call(L, 64, 2, 8, 32, 0) == -1006            # Lk < 1
    assert call(L, 64, 0, 8, 32, 40) == 0               # nothing to do
    assert call(L, 0, 2, 8, 32, 40) == 0
    assert call(L, 64, 2, 8, 32, 40) == -1001           # served shape, null q: refused before a launch
    assert call(L, 64, 2, 8, 32, 20) == -1001           # <= 32 keys are legal here too (the one-chunk path)


def test_routing_bounds_without_a_device(monkeypatch):
    """key_limit(): MAX_KEYS by default, 32 with OCPG_ATTN_LONGK=0 (the library path serves longer captions), everything the kernels can
    with =force; MAX_KEYS never exceeds what csrc/attn_longk.hip serves."""
    from ocpg_amd.models.ops.functions import attn_smallk_func as f
    assert 32 <= f.MAX_KEYS <= f.LONGK_LIMIT == 128
    monkeypatch.delenv("OCPG_ATTN_LONGK", raising=False)
    assert f.key_limit() == f.MAX_KEYS
    monkeypatch.setenv("OCPG_ATTN_LONGK", "0")
    assert f.key_limit() == 32
    monkeypatch.setenv("OCPG_ATTN_LONGK", "force")
    assert f.key_limit() == 128
