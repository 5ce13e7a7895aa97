"""csrc/lfm_dft_czt.hip without a GPU: the chirp table drives an fp64 emulation of the kernel's algorithm to torch.fft's result, the return
codes both entry points issue before any HIP call (null pointers, no device), and the routing function of models/modules.py."""
import pytest
import torch

from ocpg_amd.models.ops.functions import spectral_func as sf


@pytest.fixture(scope="module")
def L():
    from ocpg_amd import _lib
    from ocpg_amd.csrc import build
    build.build()
    return _lib.lib()


def _emulate(x, table, inverse):
    """The line transform as csrc/lfm_dft_czt.hip runs it, in fp64, from the table's contents alone: x complex [lines, n]."""
    n = x.shape[-1]
    t = torch.view_as_complex(table.double().contiguous())
    assert t.shape == (896,)
    c, b, w = t[:128], (t[384:640] if inverse else t[128:384]).reshape(16, 16), t[640:]
    if inverse:
        c = c.conj()
    i = torch.arange(16)
    f16 = w[16 * ((i[:, None] * i[None, :]) % 16)]                          # W_16^(j k) from the W_256 table
    tw = w[i[:, None] * i[None, :]]                                          # W_256^(r k1)
    a = torch.zeros(x.shape[0], 256, dtype=torch.complex128)
    a[:, :n] = x * c[:n]
    a = a.reshape(-1, 16, 16)                                                # [j, r]: element 16 j + r
    y = torch.einsum("kj,bjr->bkr", f16, a) * tw                             # first stage: slot 16 k1 + r
    big = torch.einsum("bkr,qr->bkq", y, f16)                                # A[k1 + 16 k2] at [k1, k2]
    z = torch.einsum("bkq,mq->bkm", big * b, f16.conj()) * tw.conj()         # * B, first inverse stage: slot 16 k1 + m2
    out = torch.einsum("pk,bkm->bpm", f16.conj(), z).reshape(-1, 256)        # y[16 m1 + m2]
    return out[:, :n] * c[:n]


@pytest.mark.parametrize("n", [65, 83, 106, 107, 127, 128])
def test_table_drives_the_algorithm_to_torch_fft(n):
    table = sf._twiddles_czt(n, "cpu")
    assert table.dtype == torch.float32 and table.shape == (896, 2)
    assert sf._twiddles_czt(n, "cpu") is table                                # memoised
    assert (table[n:128] == 0).all()
    torch.manual_seed(n)
    x = torch.randn(5, n, dtype=torch.complex128)
    x[0] = 0
    x[0, n - 1] = 1                                                           # the last element alone: the longest reach of the chirp
    bound = 1e-6 * x.abs().sum(-1, keepdim=True)
    for inverse in (False, True):
        ref = torch.fft.ifft(x, norm="forward") if inverse else torch.fft.fft(x)
        err = (_emulate(x, table, inverse) - ref).abs()
        assert (err <= bound).all(), (n, inverse, (err / bound).max().item())


def _fwd(L, H, W, hp, wp, cz_h=None, cz_w=None, N=2, C=8, ptr=1 << 20, dt=0, **null):
    a = dict(x=ptr, tw_h=ptr, tw_w=ptr, tmp=ptr, pair=ptr)
    a.update(null)
    return L.ocpg_lfm_spectrum_fwd_czt(a["x"], None, None, N, H, W, C, a["tw_h"], a["tw_w"], 1.0, a["tmp"], a["pair"], dt, *hp, *wp, cz_h, cz_w, None)


def _inv(L, H, W, hp, wp, cz_h=None, cz_w=None, N=2, C=8, ptr=1 << 20, dt=0, **null):
    a = dict(pair=ptr, tw_h=ptr, tw_w=ptr, tmp=ptr, out=ptr)
    a.update(null)
    return L.ocpg_lfm_spectrum_inv_czt(a["pair"], dt, None, None, None, None, N, H, W, C, a["tw_h"], a["tw_w"], 1.0, a["tmp"], None, a["out"], *hp, *wp,
                                       cz_h, cz_w, None)


@pytest.mark.parametrize("call", [_fwd, _inv], ids=["fwd", "inv"])
def test_return_codes_precede_every_hip_call(L, call):
    """Every call here either fails validation or has a null pointer, so nothing is launched (the non-null pointers are never read)."""
    cz = 1 << 20
    ok_h, ok_w = (1, 1, 23), (1, 1, 107)
    # a chirp axis: its length and the form of its plan
    for n in (64, 129, 1, 256):
        assert call(L, 23, n, ok_h, (1, 1, n), cz_w=cz) == -2000, n
        assert call(L, n, 23, (1, 1, n), ok_h, cz_h=cz) == -2000, n
    assert call(L, 23, 107, ok_h, (1, 107, 1), cz_w=cz) == -2000              # the plan of a chirp axis is (1, 1, L)
    assert call(L, 23, 106, ok_h, (1, 2, 53), cz_w=cz) == -2000
    assert call(L, 23, 107, ok_h, (1, 1, 106), cz_w=cz) == -2000
    assert call(L, 107, 23, (107, 1, 1), ok_h, cz_h=cz) == -2000
    # the other axis: whatever the _any entries refuse
    assert call(L, 23, 107, (1, 1, 22), ok_w, cz_w=cz) == -2000               # product is not H
    assert call(L, 17 * 19, 107, (1, 17, 19), ok_w, cz_w=cz) == -2000
    assert call(L, 36, 107, (1, 2, 18), ok_w, cz_w=cz) == -2000
    assert call(L, 257, 107, (1, 1, 257), ok_w, cz_w=cz) == -2000
    # without a chirp axis: the _any entries' refusals (106 = 2 * 53 is fine as a plan, 106 as one stage is not)
    assert call(L, 23, 106, ok_h, (1, 1, 106)) == -2000
    assert call(L, 23, 37, (1, 1, 22), (1, 1, 37)) == -2000
    assert call(L, 23, 107, ok_h, ok_w, cz_w=cz, N=0) == 0                    # nothing to do
    assert call(L, 23, 64, ok_h, (1, 1, 64), cz_w=cz, N=0) == 0               # (as in the _any entries: before the plans are looked at)
    assert call(L, 23, 107, ok_h, ok_w, cz_w=cz, N=-1) == (-1003 if call is _fwd else -1007)
    assert call(L, 23, 107, ok_h, ok_w, cz_w=cz, C=0) == (-1003 if call is _fwd else -1007)
    nulls = (dict(x=None), dict(tw_h=None), dict(tw_w=None), dict(tmp=None), dict(pair=None)) if call is _fwd else \
        (dict(pair=None), dict(tw_h=None), dict(tw_w=None), dict(tmp=None), dict(out=None))
    codes = (-1001, -1005, -1005, -1011, -1012) if call is _fwd else (-1001, -1011, -1011, -1014, -1016)
    for null, code in zip(nulls, codes):
        assert call(L, 23, 107, ok_h, ok_w, cz_w=cz, **null) == code, null
        assert call(L, 83, 5, (1, 1, 83), (1, 5, 1), cz_h=cz, **null) == code, null
        assert call(L, 128, 65, (1, 1, 128), (1, 1, 65), cz_h=cz, cz_w=cz, **null) == code, null
        assert call(L, 23, 106, ok_h, (1, 2, 53), **null) == code, null        # no chirp axis: the _any entries' codes
    first = dict(x=None) if call is _fwd else dict(pair=None)
    assert call(L, 23, 107, ok_h, ok_w, cz_w=cz, dt=3, **first) == -1001       # pointers before the dtype code
    from ocpg_amd import _lib
    for name in ("ocpg_lfm_spectrum_fwd_czt", "ocpg_lfm_spectrum_inv_czt"):
        assert name in _lib.SIGNATURES and name not in _lib._UNTIMED


def test_route_with_the_switch_off_is_the_parents(L, monkeypatch):
    from ocpg_amd.models import modules
    monkeypatch.setattr(modules, "DFT_CL", True)
    monkeypatch.setattr(modules, "DFT_ANY", True)
    monkeypatch.setattr(modules, "DFT_CZT", False)
    old = [bool(L.ocpg_lfm_dft_split(n)) for n in range(261)]
    anyd = [modules.dft_any_default(n) for n in range(261)]
    for h in range(1, 261):
        for w in range(1, 261):
            route, axes = modules.dft_route(h, w)
            parent = (old[h] and old[w]) or (sf.dft_any_supported(h, w) and anyd[h] and anyd[w])
            assert (route != "library") == parent and axes == (False, False), (h, w, route, axes)
            assert route == ("old" if old[h] and old[w] else "any" if parent else "library"), (h, w, route)
    for h, w in ((23, 37), (8, 34), (130, 8), (24, 40), (128, 3), (60, 107)):
        assert (old[h] and old[w]) == sf.dft_supported(h, w)                   # the table above is the predicate the block asks


def test_route_with_the_switch_on(L, monkeypatch):
    from ocpg_amd.models import modules
    monkeypatch.setattr(modules, "DFT_CL", True)
    monkeypatch.setattr(modules, "DFT_ANY", True)
    monkeypatch.setattr(modules, "DFT_CZT", True)
    monkeypatch.setattr(modules, "DFT_CZT_FORCE", False)
    monkeypatch.setattr(modules, "DFT_CZT_MIN_PRIME", 83)
    assert modules.dft_route(60, 107) == ("czt", (False, True))
    assert modules.dft_route(83, 5) == ("czt", (True, False))
    assert modules.dft_route(127, 113) == ("czt", (True, True))
    assert modules.dft_route(23, 40) == ("any", (False, False))
    assert modules.dft_route(12, 20) == ("old", (False, False))
    assert modules.dft_route(40, 134) == ("library", (False, False))           # 2 * 67: above 128 with a prime stage
    assert modules.dft_route(4, 300) == ("library", (False, False))
    assert modules.dft_route(40, 79) == ("any", (False, False))                # below the threshold: the direct stage, as before
    assert modules.dft_route(40, 106) == ("any", (False, False))               # 2 * 53 is no prime: not a chirp axis by default
    assert modules.dft_route(131, 107) == ("library", (False, False))          # the other axis must be served by default
    assert modules.dft_route(40, 67) == ("any", (False, False)) and modules.dft_route(40, 73) == ("any", (False, False))
    # no prime measured faster: the parent's routing
    monkeypatch.setattr(modules, "DFT_CZT_MIN_PRIME", None)
    assert modules.dft_route(60, 107) == ("library", (False, False)) and modules.dft_route(23, 40) == ("any", (False, False))
    # force: every prime 67..127
    monkeypatch.setattr(modules, "DFT_CZT_FORCE", True)
    assert modules.dft_route(40, 67) == ("czt", (False, True)) and modules.dft_route(79, 40) == ("czt", (True, False))
    assert modules.dft_route(40, 61) == ("any", (False, False)) and modules.dft_route(12, 20) == ("old", (False, False))
    assert modules.dft_route(60, 107) == ("czt", (False, True)) and modules.dft_route(83, 127) == ("czt", (True, True))
