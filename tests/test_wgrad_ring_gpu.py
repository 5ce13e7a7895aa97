"""The ring form of the 3x3 weight gradient (csrc/conv3x3_wgrad_ring_kernel.h: ocpg_conv3x3_mfma_wgrad_ring / _ring_h16) against the kernel
it stands in for (ocpg_conv3x3_mfma_wgrad / _h16) on the same operands.

The contract is bit identity, not a tolerance: every accumulator of the ring kernel belongs to one wave and sees the same 16-pixel k steps
in the same order as the present kernel's, so `part` is compared as raw 16-bit words.  Both outputs are pre-filled with NaN, so an element
a kernel does not write shows as a NaN that is left.  Shapes are (n, ci, co, h, w, stride), chosen from ocpg_conv3x3_mfma_wgrad_splits
(tiles = ceil(co / 64) ceil(ci / 64), splits = ceil(256 / tiles) capped by the rows) so that a workgroup really rolls its ring:
  (3, 512, 512, 7, 9, 1)     4 splits of 6 rows: workgroups cross the image boundaries at rows 7 and 14 in mid-range
  (2, 1024, 1024, 5, 6, 1)   1 split: one workgroup walks every row of both images
  (1, 1024, 1024, 4, 40, 1)  layer3's width: a 40-pixel step padded to 48
  (3, 64, 192, 4, 3, 1), (1, 128, 64, 1, 1, 1)   one row per workgroup (the ring's prologue only); maps smaller than the kernel
  (2, 72, 136, 5, 7, 1)      channel counts that are no multiples of 64
  (1, 1024, 1024, 11, 13, 2), (2, 512, 512, 6, 8, 2)   stride 2, odd and even sizes: two new rows per step
  (2, 128, 128, 9, 70, 1), (1, 256, 128, 11, 67, 2)    wider than one segment: served bit-identically or declined (-2000, part untouched)
One case also goes against F.conv2d's fp32 weight gradient on the rounded operands with the bound of
test_model_gpu.py::_conv3x3_mfma_case (rel <= 1.5e-2: bf16 partial sums, 2^-9 relative per element and split)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

NARROW = [(3, 512, 512, 7, 9, 1), (2, 1024, 1024, 5, 6, 1), (1, 1024, 1024, 4, 40, 1), (3, 64, 192, 4, 3, 1), (1, 128, 64, 1, 1, 1),
          (2, 72, 136, 5, 7, 1), (1, 1024, 1024, 11, 13, 2), (2, 512, 512, 6, 8, 2)]
WIDE = [(2, 128, 128, 9, 70, 1), (1, 256, 128, 11, 67, 2)]
_DT = {1: torch.bfloat16, 2: torch.float16}


def _operands(dev, n, ci, co, h, w, stride, dt):
    g = torch.Generator(device="cpu").manual_seed(n * 1000 + ci + 7 * h + w)
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    x = torch.randn(n, h, w, ci, generator=g).to(dev).to(_DT[dt])          # channels-last maps as the kernels read them
    gz = torch.randn(n, ho, wo, co, generator=g).to(dev).to(_DT[dt])
    return gz, x


def _both(dev, shape, dt, gz=None, x=None):
    """-> (return code of the ring symbol, part of the present kernel, part of the ring kernel), both parts pre-filled with NaN"""
    from ocpg_amd._lib import lib, stream_ptr
    L, st = lib(), stream_ptr()
    n, ci, co, h, w, stride = shape
    if gz is None:
        gz, x = _operands(dev, *shape, dt)
    sp = int(L.ocpg_conv3x3_mfma_wgrad_splits(n, h, w, ci, co, stride))
    assert sp >= 1
    p_old = torch.full((sp, co, 9 * ci), float("nan"), dtype=_DT[dt], device=dev)
    p_new = torch.full((sp, co, 9 * ci), float("nan"), dtype=_DT[dt], device=dev)
    if dt == 1:
        assert L.ocpg_conv3x3_mfma_wgrad(gz.data_ptr(), x.data_ptr(), n, h, w, ci, co, stride, p_old.data_ptr(), st) == 0
        rc = L.ocpg_conv3x3_mfma_wgrad_ring(gz.data_ptr(), x.data_ptr(), n, h, w, ci, co, stride, p_new.data_ptr(), st)
    else:
        assert L.ocpg_conv3x3_mfma_wgrad_h16(gz.data_ptr(), x.data_ptr(), n, h, w, ci, co, stride, p_old.data_ptr(), dt, st) == 0
        rc = L.ocpg_conv3x3_mfma_wgrad_ring_h16(gz.data_ptr(), x.data_ptr(), n, h, w, ci, co, stride, p_new.data_ptr(), dt, st)
    torch.cuda.synchronize()
    return rc, p_old, p_new


def _bits(t):
    return t.view(torch.int16)


@pytest.mark.parametrize("shape", NARROW)
def test_ring_is_bit_identical(dev, shape):
    rc, p_old, p_new = _both(dev, shape, 1)
    assert rc == 0
    assert not bool(torch.isnan(p_old).any()) and not bool(torch.isnan(p_new).any())
    assert torch.equal(_bits(p_old), _bits(p_new))


@pytest.mark.parametrize("shape", [NARROW[0], NARROW[6]])
def test_ring_is_bit_identical_fp16(dev, shape):
    """dtype = 2 through the _h16 symbols, and dtype = 1 through them launches what the un-suffixed symbols launch"""
    rc, p_old, p_new = _both(dev, shape, 2)
    assert rc == 0
    assert not bool(torch.isnan(p_old).any()) and not bool(torch.isnan(p_new).any())
    assert torch.equal(_bits(p_old), _bits(p_new))
    from ocpg_amd._lib import lib, stream_ptr
    L, st = lib(), stream_ptr()
    n, ci, co, h, w, stride = shape
    gz, x = _operands(dev, *shape, 1)
    _, p_ref, p_ring = _both(dev, shape, 1, gz, x)
    p_h16 = torch.full_like(p_ring, float("nan"))
    assert L.ocpg_conv3x3_mfma_wgrad_ring_h16(gz.data_ptr(), x.data_ptr(), n, h, w, ci, co, stride, p_h16.data_ptr(), 1, st) == 0
    torch.cuda.synchronize()
    assert torch.equal(_bits(p_h16), _bits(p_ring)) and torch.equal(_bits(p_h16), _bits(p_ref))


def test_ring_is_bit_identical_on_non_finite_operands(dev):
    """inf and NaN in both maps, also in the halo columns next to the padding: the same products in the same order give the same bits"""
    shape = NARROW[0]
    gz, x = _operands(dev, *shape, 1)
    x[0, 0, 0, 3] = float("inf"); x[1, 6, 8, 100] = float("-inf"); x[2, 3, 4, 511] = float("nan")
    gz[0, 6, 8, 5] = float("inf"); gz[1, 0, 0, 70] = float("nan")
    rc, p_old, p_new = _both(dev, shape, 1, gz, x)
    assert rc == 0
    assert bool(torch.isnan(p_old).any())           # the operands' own
    assert torch.equal(_bits(p_old), _bits(p_new))


@pytest.mark.parametrize("shape", WIDE)
def test_wide_maps_are_served_or_declined(dev, shape):
    rc, p_old, p_new = _both(dev, shape, 1)
    assert rc in (0, -2000)
    if rc == 0:
        assert not bool(torch.isnan(p_new).any()) and torch.equal(_bits(p_old), _bits(p_new))
    else:
        assert bool(torch.isnan(p_new).all())       # declined before any launch: untouched


def test_ring_validation_matches_the_present_symbols(dev):
    """bad dtype, null pointers, N = 0 and the geometry checks return what the present symbols return, in the same order"""
    from ocpg_amd._lib import lib, stream_ptr
    L, st = lib(), stream_ptr()
    n, ci, co, h, w, stride = 2, 64, 64, 4, 5, 1
    gz, x = _operands(dev, n, ci, co, h, w, stride, 1)
    part = torch.full((int(L.ocpg_conv3x3_mfma_wgrad_splits(n, h, w, ci, co, stride)), co, 9 * ci), 7.0, dtype=torch.bfloat16, device=dev)
    G, X, P = gz.data_ptr(), x.data_ptr(), part.data_ptr()
    calls = [(G, X, n, h, w, ci, co, stride, P, 0), (G, X, n, h, w, ci, co, stride, P, 3),       # bad dtype
             (None, None, n, h, w, ci, co, stride, None, 3),                                       # ... before the pointers
             (None, X, n, h, w, ci, co, stride, P, 1), (G, None, n, h, w, ci, co, stride, P, 1), (G, X, n, h, w, ci, co, stride, None, 1),
             (None, None, 0, h, w, ci, co, stride, None, 1), (None, None, 0, h, w, ci, co, stride, None, 2),      # N = 0: nothing to do
             (G, X, -1, h, w, ci, co, stride, P, 1), (G, X, n, 0, w, ci, co, stride, P, 1), (G, X, n, h, w, 0, co, stride, P, 1),
             (G, X, n, h, w, ci, co, 3, P, 1), (G, X, n, h, w, 60, co, stride, P, 1), (None, X, n, h, w, ci, 60, stride, P, 1)]
    for a in calls:
        want = L.ocpg_conv3x3_mfma_wgrad_h16(*a[:9], a[9], st)
        assert want != 0 or a[2] == 0, a
        assert L.ocpg_conv3x3_mfma_wgrad_ring_h16(*a[:9], a[9], st) == want, a
        if a[9] == 1:
            assert L.ocpg_conv3x3_mfma_wgrad_ring(*a[:9], st) == L.ocpg_conv3x3_mfma_wgrad(*a[:9], st) == want, a
    torch.cuda.synchronize()
    assert bool((part.float() == 7.0).all())


def test_ring_against_conv2d_weight_gradient(dev):
    shape = (3, 512, 512, 7, 9, 1)
    n, ci, co, h, w, stride = shape
    gz, x = _operands(dev, *shape, 1)
    rc, _, p_new = _both(dev, shape, 1, gz, x)
    assert rc == 0
    gw = p_new.float().sum(0).view(co, 3, 3, ci).permute(0, 3, 1, 2)
    wr = torch.zeros(co, ci, 3, 3, device=dev, requires_grad=True)
    yr = torch.nn.functional.conv2d(x.float().permute(0, 3, 1, 2), wr, None, stride, 1)
    gwr, = torch.autograd.grad(yr, wr, gz.float().permute(0, 3, 1, 2))
    rel = float((gw - gwr).norm() / (gwr.norm() + 1e-20))
    assert rel <= 1.5e-2, rel


@pytest.mark.parametrize("shape,served", [((2, 512, 512, 7, 9, 1), True), ((1, 256, 512, 11, 13, 2), True), ((2, 128, 128, 9, 70, 1), None)])
def test_switch_through_the_autograd_node(dev, shape, served, monkeypatch):
    """conv3x3_mfma_bn_act with OCPG_WGRAD_RING on and off: gw bit-identical; the census shows the ring symbol exactly when the switch is on
    and the shape is served (counted also as the symbol it stands in for: _lib.CENSUS_ALSO)"""
    from ocpg_amd import _lib
    from ocpg_amd.models.ops.functions import conv_bn_func as f
    n, ci, co, h, w, stride = shape
    if served is None:      # a wide map: served exactly when the entry point does not decline it
        served = _both(dev, shape, 1)[0] == 0
    g = torch.Generator(device="cpu").manual_seed(ci + h)
    x = torch.randn(n, ci, h, w, generator=g).to(dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    wt = (torch.randn(co, ci, 3, 3, generator=g) * (2.0 / (9 * ci)) ** 0.5).to(dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    scale, shift = (torch.rand(co, generator=g) + 0.5).to(dev), (torch.randn(co, generator=g) * 0.1).to(dev)
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    go = torch.randn(n, co, ho, wo, generator=g).to(dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    monkeypatch.setattr(f, "WGRAD_OWN", True)
    got = {}
    for on in (True, False):
        monkeypatch.setattr(f, "WGRAD_RING", on)
        xi, wi = x.clone().requires_grad_(True), wt.clone().requires_grad_(True)
        calls = _lib.census(True)
        try:
            y = f.conv3x3_mfma_bn_act(xi, wi, scale, shift, True, stride, 1)
            _, gw = torch.autograd.grad(y, (xi, wi), go)
            torch.cuda.synchronize()
        finally:
            _lib.census(False)
        got[on] = (gw.clone(), dict(calls))
        assert calls.get("ocpg_conv3x3_mfma_wgrad", 0) == 1, calls
        assert calls.get("ocpg_conv3x3_mfma_wgrad_ring", 0) == (1 if on and served else 0), calls
    assert torch.equal(_bits(got[True][0].contiguous()), _bits(got[False][0].contiguous()))
