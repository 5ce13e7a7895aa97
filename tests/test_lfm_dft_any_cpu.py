"""csrc/lfm_dft_any.hip without a GPU: the plan of every length, that the old predicate did not move, and the return codes both new
entry points issue before any HIP call (null pointers, no device)."""
import pytest

from ocpg_amd.models.ops.functions import spectral_func as sf


@pytest.fixture(scope="module")
def L():
    from ocpg_amd import _lib
    from ocpg_amd.csrc import build
    build.build()
    return _lib.lib()


def _prime(v):
    return v >= 2 and all(v % d for d in range(2, int(v ** 0.5) + 1))


def test_plan_of_every_length():
    for n in range(1, 257):
        plan = sf.dft_plan(n)
        assert isinstance(plan, tuple) and len(plan) == 3, (n, plan)
        assert plan[0] * plan[1] * plan[2] == n, (n, plan)
        big = [r for r in plan if r > 16]
        assert all(r >= 1 for r in plan) and len(big) <= 1 and all(_prime(r) and r <= 251 for r in big), (n, plan)
        assert list(plan) == sorted(plan), (n, plan)            # ascending, the 1s in front, the prime stage last
    for n in (0, -3, 257, 300, 1024):
        assert sf.dft_plan(n) is None
    # the stated rule on the lengths the header and DESIGN name
    assert sf.dft_plan(1) == (1, 1, 1) and sf.dft_plan(13) == (1, 1, 13) and sf.dft_plan(16) == (1, 1, 16)
    assert sf.dft_plan(125) == (5, 5, 5) and sf.dft_plan(250) == (5, 5, 10) and sf.dft_plan(256) == (1, 16, 16)
    assert sf.dft_plan(23) == (1, 1, 23) and sf.dft_plan(46) == (1, 2, 23) and sf.dft_plan(107) == (1, 1, 107) and sf.dft_plan(255) == (1, 15, 17)
    assert sf.dft_plan(64) == (1, 8, 8) and sf.dft_plan(80) == (1, 8, 10) and sf.dft_plan(240) == (1, 15, 16) and sf.dft_plan(128) == (1, 8, 16)
    assert sf.dft_any_supported(23, 37) and sf.dft_any_supported(256, 255) and sf.dft_any_supported(1, 1)
    assert not sf.dft_any_supported(257, 8) and not sf.dft_any_supported(8, 300) and not sf.dft_any_supported(0, 8)


def _old_split(n):
    """csrc/lfm_dft.hip's rule, restated: n = L1 * L2, both <= 16, n <= 128, the pair with the smallest sum (the smallest L1 among equals)."""
    if n < 1 or n > 128:
        return 0
    best = None
    for a in range(1, 17):
        if n % a == 0 and n // a <= 16 and (best is None or a + n // a < best[0] + best[1]):
            best = (a, n // a)
    return best[0] * 256 + best[1] if best else 0


def test_old_predicate_did_not_move(L):
    unserved = []
    for n in range(1, 301):
        assert L.ocpg_lfm_dft_split(n) == _old_split(n), n
        if n <= 128 and not _old_split(n):
            unserved.append(n)
    assert len(unserved) == 56 and 125 in unserved and all(n == 125 or any(n % p == 0 for p in range(17, 128) if _prime(p)) for n in unserved)
    for h, w in ((23, 37), (8, 34), (130, 8), (24, 40), (48, 80), (128, 3), (6, 121)):
        assert L.ocpg_lfm_dft_supported(h, w) == int(bool(_old_split(h)) and bool(_old_split(w))), (h, w)
    # an old-served axis keeps its old split as its plan under the new entries
    assert sf._axis_plan(8) == (2, 4, 1) and sf._axis_plan(13) == (1, 13, 1) and sf._axis_plan(40) == (5, 8, 1) and sf._axis_plan(34) == (1, 2, 17) and sf._axis_plan(16) == (4, 4, 1)


def _fwd(L, H, W, hp, wp, N=2, C=8, ptr=1 << 20, dt=0, **null):
    a = dict(x=ptr, tw_h=ptr, tw_w=ptr, tmp=ptr, pair=ptr)
    a.update(null)
    return L.ocpg_lfm_spectrum_fwd_any(a["x"], None, None, N, H, W, C, a["tw_h"], a["tw_w"], 1.0, a["tmp"], a["pair"], dt, *hp, *wp, None)


def _inv(L, H, W, hp, wp, N=2, C=8, ptr=1 << 20, dt=0, **null):
    a = dict(pair=ptr, tw_h=ptr, tw_w=ptr, tmp=ptr, out=ptr)
    a.update(null)
    return L.ocpg_lfm_spectrum_inv_any(a["pair"], dt, None, None, None, None, N, H, W, C, a["tw_h"], a["tw_w"], 1.0, a["tmp"], None, a["out"], *hp, *wp,
                                       None)


@pytest.mark.parametrize("call", [_fwd, _inv], ids=["fwd", "inv"])
def test_return_codes_precede_every_hip_call(L, call):
    """Every call here either fails validation or has a null pointer, so nothing is launched (the non-null pointers are never read)."""
    ok_h, ok_w = (1, 1, 23), (1, 1, 37)
    assert call(L, 23, 37, (1, 1, 22), ok_w) == -2000                   # product is not H
    assert call(L, 23, 37, ok_h, (1, 37, 2)) == -2000                   # product is not W
    assert call(L, 17 * 19, 37, (1, 17, 19), ok_w) == -2000             # two stages above 16 (and a length above 256)
    assert call(L, 23, 17 * 13, ok_h, (1, 1, 221)) == -2000             # a stage above 16 that is not a prime
    assert call(L, 23, 36, ok_h, (1, 2, 18)) == -2000                   # 18 is neither <= 16 nor a prime
    assert call(L, 23, 37, (0, 1, 23), ok_w) == -2000 and call(L, 23, 37, (-1, -1, 23), ok_w) == -2000
    assert call(L, 257, 37, (1, 1, 257), ok_w) == -2000                 # a prime, but the length is above 256
    assert call(L, 23, 512, ok_h, (2, 16, 16)) == -2000
    assert call(L, 23, 37, ok_h, ok_w, N=0) == 0                        # nothing to do
    assert call(L, 23, 37, ok_h, ok_w, N=-1) == (-1003 if call is _fwd else -1007)
    assert call(L, 23, 37, ok_h, ok_w, C=0) == (-1003 if call is _fwd else -1007)
    nulls = (dict(x=None), dict(tw_h=None), dict(tw_w=None), dict(tmp=None), dict(pair=None)) if call is _fwd else \
        (dict(pair=None), dict(tw_h=None), dict(tw_w=None), dict(tmp=None), dict(out=None))
    codes = (-1001, -1005, -1005, -1011, -1012) if call is _fwd else (-1001, -1011, -1011, -1014, -1016)
    for null, code in zip(nulls, codes):
        # the plan is valid (the 1s may stand anywhere, the old split of an old-served axis included): the pointer is what is refused
        assert call(L, 23, 37, ok_h, ok_w, **null) == code, null
        assert call(L, 8, 34, (1, 8, 1), (2, 17, 1), **null) == code, null
        assert call(L, 250, 256, (5, 5, 10), (1, 16, 16), **null) == code, null
    first = dict(x=None) if call is _fwd else dict(pair=None)
    assert call(L, 23, 37, ok_h, ok_w, dt=3, **first) == -1001          # the old entries' order: pointers before the dtype code
    from ocpg_amd import _lib
    for name in ("ocpg_lfm_spectrum_fwd_any", "ocpg_lfm_spectrum_inv_any"):
        assert name in _lib.SIGNATURES and name not in _lib._UNTIMED
