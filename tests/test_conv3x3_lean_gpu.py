"""conv3x3_mfma without the work a step does not use (csrc/conv3x3_mfma.hip, csrc/conv3x3_mfma_kernel.h):

1. the forward's patch-matrix output is a template parameter (COLS): the launch with cols == NULL (the shipped step's) and the one with
   cols given must write the same y bit for bit, the latter also the patch matrix ocpg_im2col3x3_nhwc writes;
2. the stride-2 own-weight input gradient in parity-class tiles (ocpg_conv3x3_mfma_dgrad_w_s2[_h16]) against the nine-tap symbols on the
   same operands: bit-identical dx (the same non-zero products in the same order), every element written;
3. the same through conv3x3_mfma_bn_act with the switch DGRAD_S2_CLASSES on and off.

Bounds against fp32 are the existing ones of tests/test_model_gpu.py::_conv3x3_mfma_case (rel(y) <= 6e-3, max|y - yr| <= 2e-2 max|yr| +
1e-3, rel(gx) <= 1.5e-2), in bf16 and (being bounds on a format with three more mantissa bits) in fp16 alike.  The 192 x 256 maps are the
smallest that reach the 128-column tile (ceil(rows / 64) * ceil(columns / 128) >= 768)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

CL = torch.channels_last
DTYPES = {"bf16": (torch.bfloat16, 1), "fp16": (torch.float16, 2)}


def _rel(a, b):
    a, b = a.detach().float(), b.detach().float()
    return float((a - b).norm() / (b.norm() + 1e-20))


def _bits(t):
    return t.contiguous().view(torch.int16)


@functools.lru_cache(maxsize=None)
def _operands(dname, n, c, co, h, w, stride):
    """x [n,h,w,c], weight [co,3,3,c], dy [n,ho,wo,co] in the storage type (channels-last as they lie), fp32 scale / shift per channel of
    either side, and the fp32 references on the ROUNDED operands: y = conv(x, w), gx = its input gradient for dy.  Computed once per
    shape and type and never modified."""
    dev = torch.device("cuda:0")
    dt = DTYPES[dname][0]
    g = torch.Generator(device="cpu").manual_seed(n * 1000 + c + 7 * h + w)
    x = torch.randn(n, h, w, c, generator=g).to(dev).to(dt)
    wt = (torch.randn(co, 3, 3, c, generator=g) * (2.0 / (9 * c)) ** 0.5).to(dev).to(dt)
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    dy = torch.randn(n, ho, wo, co, generator=g).to(dev).to(dt)
    sc_out, sh_out = (torch.rand(co, generator=g) + 0.5).to(dev), (torch.randn(co, generator=g) * 0.1).to(dev)
    sc_in = (torch.rand(c, generator=g) + 0.5).to(dev)
    xr = x.float().permute(0, 3, 1, 2).requires_grad_(True)
    yr = torch.nn.functional.conv2d(xr, wt.float().permute(0, 3, 1, 2), None, stride, 1)
    gxr, = torch.autograd.grad(yr, xr, dy.float().permute(0, 3, 1, 2))
    return x, wt, dy, sc_out, sh_out, sc_in, yr.detach().permute(0, 2, 3, 1).contiguous(), gxr.permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("dname", ["bf16", "fp16"])
@pytest.mark.parametrize("n,c,co,h,w,stride", [(1, 64, 64, 5, 7, 1), (2, 128, 72, 6, 8, 2), (1, 64, 68, 3, 3, 1), (1, 64, 128, 192, 256, 1)])
def test_forward_with_and_without_cols(dev, dname, n, c, co, h, w, stride):
    from ocpg_amd._lib import lib, stream_ptr
    L, st = lib(), stream_ptr()
    dt, code = DTYPES[dname]
    x, wt, _, scale, shift, _, yr, _ = _operands(dname, n, c, co, h, w, stride)
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    m = n * ho * wo
    nan = torch.full((m, co), float("nan"), dtype=dt, device=dev)
    y0, y1 = nan.clone(), nan.clone()
    cols = torch.full((m, 9 * c), float("nan"), dtype=dt, device=dev)
    ref_cols = torch.empty_like(cols)
    args = (x.data_ptr(), wt.data_ptr(), scale.data_ptr(), shift.data_ptr(), 1, n, h, w, c, co, stride)
    assert L.ocpg_conv3x3_mfma_fwd_cols_h16(*args, y0.data_ptr(), None, code, st) == 0
    assert L.ocpg_conv3x3_mfma_fwd_cols_h16(*args, y1.data_ptr(), cols.data_ptr(), code, st) == 0
    assert L.ocpg_im2col3x3_nhwc(x.data_ptr(), n, h, w, c, stride, 1, ref_cols.data_ptr(), code, st) == 0
    torch.cuda.synchronize()
    assert torch.equal(_bits(y0), _bits(y1))
    assert torch.equal(_bits(cols), _bits(ref_cols))
    ref = (yr.reshape(m, co) * scale + shift).relu()
    r, dmax, ymax = _rel(y0, ref), (y0.float() - ref).abs().max().item(), ref.abs().max().item()
    print(f"conv3x3 fwd {dname} n{n} c{c} co{co} {h}x{w} s{stride}: rel(y) {r:.3e} max|y-yr| {dmax:.3e} max|yr| {ymax:.3e}")
    assert r <= 6e-3, r
    assert dmax <= 2e-2 * ymax + 1e-3, (dmax, ymax)


@pytest.mark.parametrize("dname", ["bf16", "fp16"])
@pytest.mark.parametrize("epilogue", [True, False], ids=["mask_scale", "plain"])
@pytest.mark.parametrize("n,c,co,h,w", [(1, 64, 64, 1, 1), (1, 64, 64, 2, 2), (2, 64, 64, 5, 7), (1, 72, 128, 6, 9), (3, 128, 64, 8, 8),
                                        (1, 128, 64, 192, 256)])
def test_stride2_class_tiles_match_the_nine_tap_walk(dev, dname, epilogue, n, c, co, h, w):
    from ocpg_amd._lib import lib, stream_ptr
    L, st = lib(), stream_ptr()
    dt, code = DTYPES[dname]
    x, wt, dy, _, _, sc_in, _, gxr = _operands(dname, n, c, co, h, w, 2)
    mask_ptr, scale_ptr = (x.data_ptr(), sc_in.data_ptr()) if epilogue else (None, None)     # the mask is the convolution's own input, as in the step
    dx9 = torch.full((n, h, w, c), float("nan"), dtype=dt, device=dev)
    dxc = dx9.clone()
    args = (dy.data_ptr(), wt.data_ptr(), mask_ptr, scale_ptr, n, h, w, c, co, 2)
    assert L.ocpg_conv3x3_mfma_dgrad_w_h16(*args, dx9.data_ptr(), code, st) == 0
    assert L.ocpg_conv3x3_mfma_dgrad_w_s2_h16(*args, dxc.data_ptr(), code, st) == 0
    if code == 1:       # the un-suffixed symbol forwards to the same launch
        dxb = dx9.clone().fill_(float("nan"))
        assert L.ocpg_conv3x3_mfma_dgrad_w_s2(*args, dxb.data_ptr(), st) == 0
        assert torch.equal(_bits(dxb), _bits(dxc))
    torch.cuda.synchronize()
    assert torch.isfinite(dxc).all() and torch.isfinite(dx9).all()          # every element written
    assert torch.equal(_bits(dxc), _bits(dx9))
    ref = gxr * sc_in * (x > 0) if epilogue else gxr
    r = _rel(dxc, ref)
    print(f"conv3x3 dgrad s2 {dname} n{n} c{c} co{co} {h}x{w} epilogue={epilogue}: rel(dx) {r:.3e}")
    assert r <= 1.5e-2, r


def test_class_symbols_refuse_stride_1(dev):
    from ocpg_amd._lib import lib, stream_ptr
    L, st = lib(), stream_ptr()
    x, wt, dy, _, _, _, _, _ = _operands("bf16", 1, 64, 64, 5, 7, 1)
    dx = torch.zeros_like(x)
    assert L.ocpg_conv3x3_mfma_dgrad_w_s2(dy.data_ptr(), wt.data_ptr(), None, None, 1, 5, 7, 64, 64, 1, dx.data_ptr(), st) == -2000
    assert L.ocpg_conv3x3_mfma_dgrad_w_s2_h16(dy.data_ptr(), wt.data_ptr(), None, None, 1, 5, 7, 64, 64, 1, dx.data_ptr(), 1, st) == -2000
    assert L.ocpg_conv3x3_mfma_dgrad_w_s2_h16(dy.data_ptr(), wt.data_ptr(), None, None, 1, 5, 7, 64, 64, 2, dx.data_ptr(), 3, st) == -1010


@pytest.mark.parametrize("dname", ["bf16", "fp16"])
@pytest.mark.parametrize("n,c,co,h,w", [(1, 128, 256, 7, 9), (2, 64, 64, 6, 6)])
def test_switch_through_conv3x3_mfma_bn_act(dev, monkeypatch, dname, n, c, co, h, w):
    from ocpg_amd import _lib
    from ocpg_amd.models.ops.functions import conv_bn_func as f
    dt = DTYPES[dname][0]
    x, wt, dy, scale, shift, _, _, _ = _operands(dname, n, c, co, h, w, 2)
    xn, wn, go = x.permute(0, 3, 1, 2), wt.permute(0, 3, 1, 2), dy.permute(0, 3, 1, 2)      # channels-last views of [n,c,h,w] / [co,c,3,3]
    new = "ocpg_conv3x3_mfma_dgrad_w_s2" + ("_h16" if dname == "fp16" else "")
    res = []
    for on in (True, False):
        monkeypatch.setattr(f, "DGRAD_S2_CLASSES", on)
        xi, wi = xn.clone(memory_format=CL).requires_grad_(True), wn.clone(memory_format=CL).requires_grad_(True)
        calls = _lib.census(True)
        try:
            y = f.conv3x3_mfma_bn_act(xi, wi, scale, shift, True, 2, 1)
            gx, gw = torch.autograd.grad(y, (xi, wi), go)
            torch.cuda.synchronize()
        finally:
            _lib.census(False)
        assert calls.get(new, 0) == (1 if on else 0), calls
        assert gx.dtype == dt and gw.dtype == dt
        res.append((y.detach(), gx, gw))
    for a, b in zip(*res):
        assert torch.equal(_bits(a), _bits(b))
