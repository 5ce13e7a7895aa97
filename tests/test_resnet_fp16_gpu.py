"""The ResNet body under fp16 (the reference's --amp mode: engine.py amp.autocast + GradScaler): the fp16 forms of the frozen-BN kernel
(csrc/bn_act.hip), of the 3x3 convolution's forward / input gradient / weight gradient (csrc/conv3x3_mfma.hip, csrc/conv3x3_wgrad.hip: the
_h16 entry points) and of the fused 1x1 input gradient (csrc/gemm_dgrad_bn.hip, dtype 2); the guard that keeps fp16 bits away from bf16
instantiations; a tiny training step with GradScaler and its whole-step graph.

Bounds.  fp16 has three more mantissa bits than bf16 (unit roundoff 2^-11 against 2^-8), so every bound below is the bf16 test's bound
times 2^-3, as the bf16 tests' docstrings derive theirs from the storage format's rounding:
  frozen BN                    rtol = atol = 2e-3              (test_bn_act_gpu.py: 1.6e-2)
  conv3x3 rel(y)               7.5e-4                          (test_model_gpu.py::_conv3x3_mfma_case: 6e-3)
  conv3x3 rel(gx), rel(gw)     1.9e-3                          (there: 1.5e-2)
  conv3x3 max|y - yr|          2.5e-3 max|yr| + 1e-3           (there: 2e-2 max|yr| + 1e-3)
  gemm_dgrad_bn                2 fp16 ulps per element, 2^-11 + 1e-6 in norm   (test_dgrad_bn_gpu.py: 2 bf16 ulps, 2^-8 + 1e-6)
A CPU emulation (fp32 convolution on the rounded operands, y, gz, gx, gw rounded to the storage type) gives rel(y) = 2.1e-4 and
rel(gx), rel(gw) = 2.9e-4 for fp16 against 1.7e-3 and 2.3e-3 for bf16: the same 3.6x and 6.4x head-room on both sides."""
import math
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

H16 = torch.float16
CL = torch.channels_last


def _ptr(t):
    return None if t is None else t.data_ptr()


def _rel(a, b):
    a, b = a.detach().float(), b.detach().float()
    return float((a - b).norm() / (b.norm() + 1e-20))


# ---- 1. frozen BN (+ skip) (+ ReLU) -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["nhwc", "nchw"])
@pytest.mark.parametrize("shape", [(2, 64, 12, 20), (3, 256, 7, 5), (1, 24, 3, 3), (2, 2048, 12, 20)])
@pytest.mark.parametrize("with_skip,relu", [(False, True), (True, True), (False, False)])
def test_bn_act_fp16_matches_reference(dev, layout, shape, with_skip, relu):
    """The grid of test_bn_act_gpu.py::test_bn_act_matches_reference (both layouts; its four shapes: the vector paths and, NCHW 3 x 3, the
    scalar one) in torch.float16 against the same fp32 CPU reference; rtol = atol = 2e-3 = the bf16 test's 1.6e-2 times 2^-3."""
    from test_bn_act_gpu import _ref
    from ocpg_amd.models.backbone import FrozenBatchNorm2d
    g = torch.Generator().manual_seed(sum(shape))
    n, c, h, w = shape
    bn = FrozenBatchNorm2d(c)
    bn.weight.copy_(1 + 0.1 * torch.randn(c, generator=g)); bn.bias.copy_(0.1 * torch.randn(c, generator=g))
    bn.running_mean.copy_(0.1 * torch.randn(c, generator=g)); bn.running_var.copy_(torch.rand(c, generator=g) + 0.5)
    x = torch.randn(shape, generator=g).to(H16)
    skip = torch.randn(shape, generator=g).to(H16) if with_skip else None
    go = torch.randn(shape, generator=g).to(H16)
    xr = x.float().clone().requires_grad_(True)
    sr = skip.float().clone().requires_grad_(True) if with_skip else None
    yr = _ref(xr, bn.weight, bn.bias, bn.running_mean, bn.running_var, sr, relu)
    yr.backward(go.float())
    fmt = CL if layout == "nhwc" else torch.contiguous_format
    bn.to(dev)
    xd = x.to(dev).contiguous(memory_format=fmt).requires_grad_(True)
    sd = skip.to(dev).contiguous(memory_format=fmt).requires_grad_(True) if with_skip else None
    y = bn(xd, skip=sd, relu=relu)
    assert y.dtype == H16 and y.stride() == xd.stride()
    y.backward(go.to(dev).contiguous(memory_format=fmt))
    tol = dict(rtol=2e-3, atol=2e-3)
    print("bn_act fp16 %s %s skip=%s relu=%s: max|y - yr| %.3e" % (layout, shape, with_skip, relu, (y.detach().cpu().float() - yr.detach()).abs().max().item()))
    assert torch.allclose(y.detach().cpu().float(), yr.detach(), **tol)
    # gradient masks come from the fp16-rounded output: compare away from the ReLU kink, as the bf16 test does
    safe = (yr.detach().abs() > 0.05) if relu else torch.ones_like(yr, dtype=torch.bool)
    assert torch.allclose(xd.grad.cpu().float()[safe], xr.grad[safe], **tol)
    if with_skip:
        assert torch.allclose(sd.grad.cpu().float()[safe], sr.grad[safe], **tol)


def test_bn_act_fp16_nan_inf_and_overflow_pass_through(dev):
    """NaN and inf pass through, a result past 65504 becomes inf (as ATen's cast does; the GradScaler deals with it): no clamping."""
    from ocpg_amd.models.ops.functions.bn_act_func import frozen_bn_act
    x = torch.tensor([1.0, float("nan"), float("inf"), -float("inf"), 60000.0, -60000.0, 3.0, -3.0], dtype=H16, device=dev).view(1, 8, 1, 1)
    scale, shift = torch.full((8,), 2.0, device=dev), torch.zeros(8, device=dev)
    y = frozen_bn_act(x, scale, shift, None, False).flatten().float().cpu()
    assert y[0] == 2.0 and math.isnan(y[1]) and y[2] == math.inf and y[3] == -math.inf and y[4] == math.inf and y[5] == -math.inf
    assert y[6] == 6.0 and y[7] == -6.0


# ---- 2. conv3x3 forward / input gradient / weight gradient -----------------------------------------------------------------------
def _conv3x3_inputs(dev, n, c, co, h, w, stride, dtype):
    g = torch.Generator(device="cpu").manual_seed(n * 1000 + c + h)
    x = torch.randn(n, c, h, w, generator=g).to(dev).to(dtype).contiguous(memory_format=CL)
    wt = (torch.randn(co, c, 3, 3, generator=g) * (2.0 / (9 * c)) ** 0.5).to(dev).to(dtype).contiguous(memory_format=CL)
    scale = (torch.rand(co, generator=g) + 0.5).to(dev)
    shift = (torch.randn(co, generator=g) * 0.1).to(dev)
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    go = torch.randn(n, co, ho, wo, generator=g).to(dev).to(dtype).contiguous(memory_format=CL)
    return x, wt, scale, shift, go


def _conv3x3_fp16_case(dev, n, c, co, h, w, stride, relu, monkeypatch):
    """The protocol of test_model_gpu.py::_conv3x3_mfma_case in fp16: F.conv2d in fp32 on the same fp16-rounded operands plus the affine."""
    from ocpg_amd import _lib
    from ocpg_amd.models.ops.functions import conv_bn_func as f
    monkeypatch.setattr(f, "DGRAD_OWN_WEIGHT", True)
    monkeypatch.setattr(f, "WGRAD_OWN", True)
    x, wt, scale, shift, go = _conv3x3_inputs(dev, n, c, co, h, w, stride, H16)
    ho, wo = go.shape[2], go.shape[3]
    xi, wi = x.clone().requires_grad_(True), wt.clone().requires_grad_(True)
    calls = _lib.census(True)
    try:
        y = f.conv3x3_mfma_bn_act(xi, wi, scale, shift, relu, stride, 1)
        assert y.shape == (n, co, ho, wo) and y.is_contiguous(memory_format=CL) and y.dtype == H16
        gx, gw = torch.autograd.grad(y, (xi, wi), go)
        torch.cuda.synchronize()
    finally:
        _lib.census(False)
    assert calls.get("ocpg_conv3x3_mfma_fwd_cols_h16") == 1 and calls.get("ocpg_conv3x3_mfma_dgrad_w_h16") == 1, calls
    assert calls.get("ocpg_conv3x3_mfma_wgrad_h16") == 1, calls
    assert not [k for k in calls if k.startswith("ocpg_conv3x3_mfma_") and not k.endswith("_h16") and "splits" not in k], calls
    assert gx.dtype == H16 and gw.dtype == H16
    xr, wr = x.float().requires_grad_(True), wt.float().requires_grad_(True)
    yr = torch.nn.functional.conv2d(xr, wr, None, stride, 1) * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
    yr = yr.relu() if relu else yr
    gxr, gwr = torch.autograd.grad(yr, (xr, wr), go.float())
    ry, rgx, rgw = _rel(y, yr), _rel(gx, gxr), _rel(gw, gwr)
    dmax, ymax = (y.float() - yr).abs().max().item(), yr.abs().max().item()
    print(f"conv3x3 fp16 n{n} c{c} co{co} {h}x{w} s{stride} relu={relu}: rel(y) {ry:.3e} rel(gx) {rgx:.3e} rel(gw) {rgw:.3e} max|y-yr| {dmax:.3e} max|yr| {ymax:.3e}")
    assert ry <= 7.5e-4, ry
    assert rgx <= 1.9e-3, rgx
    assert rgw <= 1.9e-3, rgw
    assert dmax <= 2.5e-3 * ymax + 1e-3, (dmax, ymax)


@pytest.mark.parametrize("n,c,co,h,w,stride", [(10, 256, 256, 24, 40, 1), (2, 128, 128, 48, 80, 1), (3, 256, 256, 48, 80, 2),
                                                (2, 512, 512, 12, 20, 1), (1, 128, 256, 7, 9, 2), (2, 192, 320, 5, 6, 1)])
@pytest.mark.parametrize("relu", [True, False])
def test_conv3x3_fp16_kernels(dev, n, c, co, h, w, stride, relu, monkeypatch):
    """The shapes of test_conv3x3_mfma_kernel: ResNet-101 layer2/3/4 with both strides (64- and 128-column tiles), the ragged 7 x 9 map and
    channel counts that are not multiples of 128."""
    _conv3x3_fp16_case(dev, n, c, co, h, w, stride, relu, monkeypatch)


@pytest.mark.parametrize("n,c,co,h,w,stride", [(2, 128, 128, 9, 70, 1), (1, 256, 128, 11, 67, 2), (3, 64, 192, 4, 3, 1), (1, 128, 64, 1, 1, 1)])
def test_conv3x3_fp16_segments_and_ragged_maps(dev, n, c, co, h, w, stride, monkeypatch):
    """Maps wider than one 64- / 32-pixel segment of the weight-gradient kernel, odd sizes under stride 2, maps smaller than the kernel."""
    _conv3x3_fp16_case(dev, n, c, co, h, w, stride, True, monkeypatch)


def test_conv3x3_fp16_forward_writes_the_patch_matrix(dev):
    """OCPG_CONV3X3_FWD_COLS stays allowed in fp16: the cols output of the fp16 forward is what ocpg_im2col3x3_nhwc writes."""
    from ocpg_amd._lib import lib, stream_ptr
    L, st = lib(), stream_ptr()
    n, c, co, h, w, stride = 2, 128, 192, 9, 11, 2
    x, wt, scale, shift, _ = _conv3x3_inputs(dev, n, c, co, h, w, stride, H16)
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    w2 = wt.permute(0, 2, 3, 1).contiguous()
    y0 = torch.empty(n, co, ho, wo, dtype=H16, device=dev).contiguous(memory_format=CL)
    y1 = torch.empty_like(y0)
    cols = torch.full((n * ho * wo, 9 * c), 7.0, dtype=H16, device=dev)
    want = torch.empty_like(cols)
    assert L.ocpg_conv3x3_mfma_fwd_cols_h16(_ptr(x), _ptr(w2), _ptr(scale), _ptr(shift), 1, n, h, w, c, co, stride, _ptr(y0), None, 2, st) == 0
    assert L.ocpg_conv3x3_mfma_fwd_cols_h16(_ptr(x), _ptr(w2), _ptr(scale), _ptr(shift), 1, n, h, w, c, co, stride, _ptr(y1), _ptr(cols), 2, st) == 0
    assert L.ocpg_im2col3x3_nhwc(_ptr(x), n, h, w, c, stride, 1, _ptr(want), 2, st) == 0
    torch.cuda.synchronize()
    assert torch.equal(y0, y1) and torch.equal(cols, want)


# ---- 3. the _h16 symbols ----------------------------------------------------------------------------------------------------------
def test_h16_symbols_with_dtype_1_are_the_old_symbols_and_reject_other_codes(dev):
    """dtype 1 launches the very bf16 instantiation of the un-suffixed symbol (torch.equal results, one shape per kernel); dtype 0 and 3
    return -1010 before any launch: a poisoned output buffer stays untouched."""
    from ocpg_amd._lib import lib, stream_ptr
    L, st = lib(), stream_ptr()
    n, c, co, h, w, stride = 2, 128, 192, 10, 12, 1
    bf = torch.bfloat16
    x, wt, scale, shift, go = _conv3x3_inputs(dev, n, c, co, h, w, stride, bf)
    w2 = wt.permute(0, 2, 3, 1).contiguous()
    m = n * h * w
    new = lambda *s: torch.full(s, 7.0, dtype=bf, device=dev)      # noqa: E731
    # forward (+ cols)
    y_a, y_b, cols_a, cols_b = new(m, co), new(m, co), new(m, 9 * c), new(m, 9 * c)
    assert L.ocpg_conv3x3_mfma_fwd_cols(_ptr(x), _ptr(w2), _ptr(scale), _ptr(shift), 1, n, h, w, c, co, stride, _ptr(y_a), _ptr(cols_a), st) == 0
    assert L.ocpg_conv3x3_mfma_fwd_cols_h16(_ptr(x), _ptr(w2), _ptr(scale), _ptr(shift), 1, n, h, w, c, co, stride, _ptr(y_b), _ptr(cols_b), 1, st) == 0
    # input gradient from the own weight, with the mask / scale epilogue
    gz = go.permute(0, 2, 3, 1).contiguous()
    dx_a, dx_b = new(m, c), new(m, c)
    sc_in = (torch.rand(c, device=dev) + 0.5)
    assert L.ocpg_conv3x3_mfma_dgrad_w(_ptr(gz), _ptr(w2), _ptr(x), _ptr(sc_in), n, h, w, c, co, stride, _ptr(dx_a), st) == 0
    assert L.ocpg_conv3x3_mfma_dgrad_w_h16(_ptr(gz), _ptr(w2), _ptr(x), _ptr(sc_in), n, h, w, c, co, stride, _ptr(dx_b), 1, st) == 0
    # weight gradient
    sp = int(L.ocpg_conv3x3_mfma_wgrad_splits(n, h, w, c, co, stride))
    p_a, p_b = new(sp, co, 9 * c), new(sp, co, 9 * c)
    assert L.ocpg_conv3x3_mfma_wgrad(_ptr(gz), _ptr(x), n, h, w, c, co, stride, _ptr(p_a), st) == 0
    assert L.ocpg_conv3x3_mfma_wgrad_h16(_ptr(gz), _ptr(x), n, h, w, c, co, stride, _ptr(p_b), 1, st) == 0
    torch.cuda.synchronize()
    assert torch.equal(y_a, y_b) and torch.equal(cols_a, cols_b) and torch.equal(dx_a, dx_b) and torch.equal(p_a, p_b)
    assert bool((y_a.float() != 7.0).any()) and bool((dx_a.float() != 7.0).any()) and bool((p_a.float() != 7.0).any())
    for bad in (0, 3):
        y_p, cols_p, dx_p, p_p = new(m, co), new(m, 9 * c), new(m, c), new(sp, co, 9 * c)
        assert L.ocpg_conv3x3_mfma_fwd_cols_h16(_ptr(x), _ptr(w2), _ptr(scale), _ptr(shift), 1, n, h, w, c, co, stride, _ptr(y_p), _ptr(cols_p), bad,
                                                st) == -1010
        assert L.ocpg_conv3x3_mfma_dgrad_w_h16(_ptr(gz), _ptr(w2), _ptr(x), _ptr(sc_in), n, h, w, c, co, stride, _ptr(dx_p), bad, st) == -1010
        assert L.ocpg_conv3x3_mfma_wgrad_h16(_ptr(gz), _ptr(x), n, h, w, c, co, stride, _ptr(p_p), bad, st) == -1010
        torch.cuda.synchronize()
        for t in (y_p, cols_p, dx_p, p_p):
            assert bool((t.float() == 7.0).all())


# ---- 4. ocpg_gemm_dgrad_bn, dtype 2 ------------------------------------------------------------------------------------------------
def _dgrad_bn_call(a, w, c, mask, scale, out, out_skip, dtype=2, tile=None):
    from ocpg_amd._lib import lib, stream_ptr
    L = lib()
    m, k = a.shape
    n = w.shape[1]
    t = int(L.ocpg_gemm_dgrad_bn_tile(m, n, k)) if tile is None else tile
    return L.ocpg_gemm_dgrad_bn(_ptr(a), _ptr(w), _ptr(c), _ptr(mask), _ptr(scale), _ptr(out), _ptr(out_skip), m, n, k, dtype, t, stream_ptr())


def _ulps_fp16(x, ref):
    """|x - ref| in units of the fp16 spacing at |ref| (ref rounded to fp16 first): 2^(floor(log2|r|) - 10)."""
    r = ref.to(H16).float()
    spacing = torch.where(r == 0, torch.full_like(r, 2.0 ** -24), 2.0 ** (torch.floor(torch.log2(r.abs())) - 10))
    return (x.float() - r).abs() / spacing


def _dgrad_cases():
    from test_dgrad_bn_gpu import CASES
    return CASES


@pytest.mark.parametrize("mode", ["a", "b", "plain"])
@pytest.mark.parametrize("name,m,n,k", _dgrad_cases())
def test_gemm_dgrad_bn_fp16_against_fp32(dev, mode, name, m, n, k):
    """test_dgrad_bn_gpu.py::test_kernel_against_fp32 with fp16 operands and dtype 2: <= 2 fp16 ulps per element where |ref| > 1e-2 max|ref|,
    and a norm-relative error of at most 2^-11 (fp16's unit roundoff) + 1e-6."""
    g = torch.Generator().manual_seed(m + n + k)
    a = torch.randn(m, k, generator=g).to(dev, H16)
    w = (torch.randn(k, n, generator=g) / k ** 0.5).to(dev, H16)
    mask = torch.randn(m, n, generator=g).to(dev, H16)
    scale = (torch.rand(n, generator=g) + 0.5).to(dev)
    c = torch.randn(m, n, generator=g).to(dev, H16)
    v = a.float() @ w.float()
    out = torch.empty(m, n, dtype=H16, device=dev)
    if mode == "a":
        assert _dgrad_bn_call(a, w, None, mask, scale, out, None) == 0
        refs = [(out, torch.where(mask.float() > 0, v, torch.zeros_like(v)) * scale)]
    elif mode == "b":
        c0 = c.clone()
        assert _dgrad_bn_call(a, w, c, mask, scale, out, c) == 0                 # out_skip over C, in place
        mm = torch.where(mask.float() > 0, v + c0.float(), torch.zeros_like(v))
        refs = [(c, mm), (out, mm * scale)]
    else:
        assert _dgrad_bn_call(a, w, None, None, None, out, None) == 0
        refs = [(out, v)]
    torch.cuda.synchronize()
    for got, ref in refs:
        u = _ulps_fp16(got, ref)
        big = ref.abs() > 1e-2 * ref.abs().max()
        nerr = (got.float() - ref).norm().item() / ref.norm().item()
        print(f"gemm_dgrad_bn fp16 {name} m{m} n{n} k{k} {mode}: max ulps {u[big].max().item():.3f}, norm-relative {nerr:.3e}")
        assert u[big].max().item() <= 2.0, (name, mode, u[big].max().item())
        assert (got.float() - ref).norm().item() <= 2.0 ** -11 * ref.norm().item() + 1e-6


@pytest.mark.parametrize("name,m,n,k", _dgrad_cases())
def test_gemm_dgrad_bn_fp16_tiles_agree(dev, name, m, n, k):
    """As test_tiles_agree_and_fill_the_chip: every tile computes each element as the same fp32 chain over k, so the three fp16 tiles give
    the same bits (mode b: C in place, mask, scale)."""
    sizes = {0: (128, 128), 1: (64, 128), 2: (64, 64)}
    tiles = [t for t, (tm, tn) in sizes.items() if n % tn == 0]
    g = torch.Generator().manual_seed(3)
    a = torch.randn(m, k, generator=g).to(dev, H16)
    w = (torch.randn(k, n, generator=g) / k ** 0.5).to(dev, H16)
    mask = torch.randn(m, n, generator=g).to(dev, H16)
    scale = (torch.rand(n, generator=g) + 0.5).to(dev)
    c0 = torch.randn(m, n, generator=g).to(dev, H16)
    res = []
    for tile in sorted(tiles):
        c = c0.clone()
        out = torch.empty(m, n, dtype=H16, device=dev)
        assert _dgrad_bn_call(a, w, c, mask, scale, out, c, tile=tile) == 0
        res.append((out, c))
    torch.cuda.synchronize()
    assert len(res) == 3
    for out, c in res[1:]:
        assert torch.equal(out, res[0][0]) and torch.equal(c, res[0][1])


def test_gemm_dgrad_bn_still_declines_fp32(dev):
    a = torch.zeros(64, 256, dtype=H16, device=dev)
    w = torch.zeros(256, 256, dtype=H16, device=dev)
    out = torch.full((64, 256), 7.0, dtype=H16, device=dev)
    assert _dgrad_bn_call(a, w, None, None, None, out, None, dtype=0, tile=0) == -2002
    assert _dgrad_bn_call(a, w, None, None, None, out, None, dtype=3, tile=0) == -2002
    torch.cuda.synchronize()
    assert bool((out.float() == 7.0).all())


# ---- 5. no fp16 tensor reaches a bf16 instantiation (and the reverse) ------------------------------------------------------------
def _run_chain(seq, x, go, monkeypatch, **switches):
    from ocpg_amd import _lib
    from ocpg_amd.models.ops.functions import conv_bn_func
    with monkeypatch.context() as mp:
        for k, v in switches.items():
            mp.setattr(conv_bn_func, k, v)
        conv_bn_func.reset_skip_tokens()
        xi = x.clone().requires_grad_(True)
        seq.zero_grad()
        calls = _lib.census(True)
        try:
            y = seq(xi)
            y.backward(go)
            torch.cuda.synchronize()
        finally:
            counts = dict(calls)
            _lib.census(False)
        return [y.detach().float(), xi.grad.float()] + [p.grad.float() for p in seq.parameters()], counts


_CONV3X3_PLAIN = ("ocpg_conv3x3_mfma_fwd", "ocpg_conv3x3_mfma_fwd_cols", "ocpg_conv3x3_mfma_dgrad", "ocpg_conv3x3_mfma_dgrad_masked",
                  "ocpg_conv3x3_mfma_dgrad_w", "ocpg_conv3x3_mfma_wgrad", "ocpg_conv3x3_mfma_fwd_bn_splitk", "ocpg_conv3x3_mfma_dgrad_w_splitk",
                  "ocpg_conv3x3_mfma_fwd_splitk")
_CONV3X3_H16 = ("ocpg_conv3x3_mfma_fwd_cols_h16", "ocpg_conv3x3_mfma_dgrad_w_h16", "ocpg_conv3x3_mfma_wgrad_h16")


def test_fp16_chain_never_reaches_a_bf16_kernel(dev, monkeypatch):
    """The bottleneck chain of test_dgrad_bn_gpu.py (a projecting block and three identity ones at layer3's width, 10 frames of 24 x 40) cast
    to fp16, with the fused switches (FUSED_DGRAD_BN, PREMASK) on and off: the two runs agree within the conv3x3 bounds above (their
    forwards are bit-identical, so both backwards see the same ReLU masks), and the census shows the three _h16 conv symbols and
    ocpg_gemm_dgrad_bn and no un-suffixed conv3x3 symbol.  A bf16 chain shows no _h16 conv symbol.
    go carries a factor 2^-4 (exact in both formats): the weight gradients sum 9600 pixels and stay far inside fp16's range.

    With DGRAD_OWN_WEIGHT off (a path that has no fp16 form) the fp16 chain runs through the library fallback, bn(conv(x)): no conv3x3
    symbol at all in the census, a forward within the conv3x3 rel(y) bound of the fused run, finite gradients.  Its GRADIENTS cannot be
    held to the bit-level bound against the fused run: the fallback rounds the convolution to fp16 BEFORE the BN affine (as the reference
    does under autocast), the fused kernel after it, so the two forwards differ by rounding (measured rel(y) 3.8e-4) and with them the ReLU
    mask of every output closer to zero than that difference: a fraction ~ rel(y) of the elements, whose gradients are switched on in one
    run and off in the other, i.e. a norm-relative gradient difference ~ sqrt(rel(y)) ~ 2e-2 however exact the kernels are (measured
    0.9e-2 ... 2.7e-2 per tensor; the fused run itself is 0.9e-2 ... 2.4e-2 from an fp32 run of the same chain for the same reason, the
    fallback 0.9e-2 ... 2.8e-2).  The yardstick for the fallback's gradients is therefore the fp32 run of the same chain (same
    fp16-rounded weights and inputs): each of the two fp16 paths is at most twice as far from it as the other one, tensor by tensor (the
    factor of test_msda_h16_gpu.py's referee).  Misread bits would be O(1) on either side of that."""
    import copy
    from test_dgrad_bn_gpu import _chain
    seq = _chain(dev, 256, 4).to(H16)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(10, 512, 48, 80, generator=g).to(dev).to(H16).contiguous(memory_format=CL)
    go = (torch.randn(10, 1024, 24, 40, generator=g) / 16).to(dev).to(H16).contiguous(memory_format=CL)
    on, c_on = _run_chain(seq, x, go, monkeypatch, FUSED_DGRAD_BN=True, PREMASK=True)
    off, c_off = _run_chain(seq, x, go, monkeypatch, FUSED_DGRAD_BN=False, PREMASK=False)
    fb, c_fb = _run_chain(seq, x, go, monkeypatch, DGRAD_OWN_WEIGHT=False)
    for counts in (c_on, c_off):
        assert all(counts.get(k, 0) == 4 for k in _CONV3X3_H16), counts
        assert not [k for k in _CONV3X3_PLAIN if counts.get(k, 0)], counts
    assert c_on.get("ocpg_gemm_dgrad_bn", 0) == 7 and c_off.get("ocpg_gemm_dgrad_bn", 0) == 0, (c_on, c_off)
    assert not [k for k in _CONV3X3_PLAIN + _CONV3X3_H16 if c_fb.get(k, 0)], c_fb           # the library path: bn(conv(x))
    assert c_fb.get("ocpg_bn_act_fwd", 0) >= 4, c_fb
    assert all(torch.isfinite(t).all() for t in on + off + fb)
    ry = _rel(off[0], on[0])
    rg = [_rel(a, b_) for a, b_ in zip(off[1:], on[1:])]
    print(f"fp16 chain, switches off against fused: rel(y) {ry:.3e}, max rel(grad) {max(rg):.3e}")
    assert ry <= 7.5e-4, ry
    assert max(rg) <= 1.9e-3, rg
    ry = _rel(fb[0], on[0])
    print(f"fp16 chain, fallback against fused: rel(y) {ry:.3e}")
    assert ry <= 7.5e-4, ry
    ref, _ = _run_chain(copy.deepcopy(seq).float(), x.float(), go.float(), monkeypatch)      # fp32 modules, the same rounded operands
    names = ["y", "gx"] + [k for k, _ in seq.named_parameters()]
    for name, r, a, b_ in zip(names, ref, on, fb):
        d_on, d_fb = _rel(a, r), _rel(b_, r)
        print(f"fp16 chain {name}: fused against fp32 {d_on:.3e}, fallback against fp32 {d_fb:.3e}, fallback against fused {_rel(b_, a):.3e}")
        assert d_fb <= 2.0 * d_on and d_on <= 2.0 * d_fb, (name, d_on, d_fb)
    seq_bf = _chain(dev, 256, 4)
    _, c_bf = _run_chain(seq_bf, x.to(torch.bfloat16), go.to(torch.bfloat16), monkeypatch)
    assert not [k for k in _CONV3X3_H16 if c_bf.get(k, 0)], c_bf
    assert c_bf.get("ocpg_conv3x3_mfma_fwd_cols", 0) == 4 and c_bf.get("ocpg_conv3x3_mfma_dgrad_w", 0) == 4, c_bf


def test_bf16_map_stays_eligible_under_the_bf16_only_switches(dev, monkeypatch):
    """OCPG_DGRAD_OWN_WEIGHT=0 and OCPG_CONV3X3_SPLITK take only the fp16 map off the own kernels: an eligible bf16 map of the same shape
    keeps its answer under both, an fp16 one becomes ineligible."""
    from ocpg_amd.models.ops.functions import conv_bn_func as f
    conv = torch.nn.Conv2d(128, 128, 3, padding=1, bias=False)
    maps = {dt: torch.zeros(1, 128, 8, 8, device=dev, dtype=dt).contiguous(memory_format=CL) for dt in (torch.bfloat16, H16)}
    assert f.eligible3x3_mfma(maps[torch.bfloat16], conv) and f.eligible3x3_mfma(maps[H16], conv)
    for name, value in (("DGRAD_OWN_WEIGHT", False), ("BODY_SPLITK", True)):
        with monkeypatch.context() as mp:
            mp.setattr(f, name, value)
            assert f.eligible3x3_mfma(maps[torch.bfloat16], conv), name
            assert not f.eligible3x3_mfma(maps[H16], conv), name


def test_mixed_16_bit_operands_are_refused(dev):
    """An fp16 map with a bf16 weight (or the reverse) is an error of the fused node, never a launch that misreads bits."""
    from ocpg_amd.models.ops.functions import conv_bn_func as f
    x = torch.randn(1, 128, 8, 8, device=dev).to(H16).contiguous(memory_format=CL)
    wt = torch.randn(128, 128, 3, 3, device=dev).to(torch.bfloat16).contiguous(memory_format=CL)
    scale, shift = torch.ones(128, device=dev), torch.zeros(128, device=dev)
    with pytest.raises(RuntimeError, match="16-bit dtype"):
        f.conv3x3_mfma_bn_act(x, wt, scale, shift, True, 1, 1)
    with pytest.raises(RuntimeError, match="16-bit dtype"):
        f.conv3x3_mfma_bn_act(x.to(torch.bfloat16), wt.to(H16), scale, shift, True, 1, 1)


# ---- 6. / 7. the tiny ResNet model under fp16 autocast + GradScaler ---------------------------------------------------------------
def _paths():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "tests"), os.path.join(root, "tests", "golden")):
        if p not in sys.path:
            sys.path.insert(0, p)


def _tiny(dev):
    _paths()
    import model_checks
    from conftest import Golden
    meta = Golden("e2e_tiny").meta
    args, model, crit = model_checks.build_product(meta, dev)
    model_checks.to_channels_last(model)
    model.train(), crit.train()
    return meta, args, model, crit


def _tiny_batch(meta, dev):
    import cases
    import model_checks
    B, T, H, W = meta.get("B", 2), meta["T"], meta["H"], meta["W"]
    x, mask, targets = cases.e2e_inputs(B, T, H, W, meta["nopad_sizes"], dev)
    return x, mask, targets, model_checks.text_for(B, dev)


def test_tiny_resnet_training_step_under_fp16_autocast(dev):
    """The ResNet fixture e2e_tiny under torch.autocast("cuda", dtype=torch.float16) with GradScaler(init_scale=64.0) (the scale of the
    existing fp16 tests: 65536 overflows the tiny model's fp16 backward): bench.forward_backward, then one bench.EagerStep.  A finite loss
    within 2e-2 relative of the fp32 run of the same model and batch (the bound test_full_size_step_vs_oracle allows bf16; fp16 has three
    more bits), a finite gradient for every parameter that has one in the bf16 run, and the weights move."""
    _paths()
    import bench
    from ocpg_amd import _lib
    from ocpg_amd.util.misc import NestedTensor
    meta, args, model, crit = _tiny(dev)
    _, _, m_bf, c_bf = _tiny(dev)
    _, _, m_32, c_32 = _tiny(dev)
    x, mask, targets, text = _tiny_batch(meta, dev)
    c_bf.iter = 0
    bench.forward_backward(m_bf, c_bf, NestedTensor(x.clone(), mask.clone()), text, targets, torch.bfloat16)
    have = {k for k, p in m_bf.named_parameters() if p.grad is not None}
    c_32.iter = 0
    loss32 = float(bench.forward_backward(m_32, c_32, NestedTensor(x.clone(), mask.clone()), text, targets, None))
    scaler = torch.amp.GradScaler("cuda", init_scale=64.0)
    crit.iter = 0
    calls = _lib.census(True)
    try:
        loss = bench.forward_backward(model, crit, NestedTensor(x.clone(), mask.clone()), text, targets, H16, scaler=scaler)
        torch.cuda.synchronize()
    finally:
        _lib.census(False)
    print(f"tiny ResNet step: fp16 loss {float(loss):.6f}, fp32 loss {loss32:.6f}, relative {abs(float(loss) - loss32) / abs(loss32):.3e}; "
          f"census {dict((k, v) for k, v in calls.items() if 'bn_act' in k or 'conv3x3' in k or 'dgrad_bn' in k)}")
    assert torch.isfinite(loss), loss
    assert calls.get("ocpg_bn_act_fwd", 0) > 0, calls               # the frozen-BN kernel served the fp16 body
    assert abs(float(loss) - loss32) <= 2e-2 * abs(loss32), (float(loss), loss32)
    got = {k: p.grad for k, p in model.named_parameters() if p.grad is not None}
    assert have and have <= set(got), sorted(have - set(got))
    bad = [k for k in have if not torch.isfinite(got[k]).all()]
    assert not bad, bad
    before = {k: p.detach().clone() for k, p in model.named_parameters() if p.requires_grad}
    crit.iter = 0
    opt = bench.make_optimizer(model, args, fused=False)
    step = bench.EagerStep(model, model, crit, opt, lambda: NestedTensor(x.clone(), mask.clone()), text, targets, args, H16)
    assert step.scaler is not None
    step.scaler = torch.amp.GradScaler("cuda", init_scale=64.0)
    assert math.isfinite(float(step()))
    moved = {k for k, p in model.named_parameters() if p.requires_grad and not torch.equal(p.detach(), before[k])}
    body = [k for k in before if k in have and "backbone" in k]
    assert body, sorted(before)[:8]
    assert set(body) <= moved, sorted(set(body) - moved)


def test_whole_step_graph_matches_eager_under_fp16_resnet(dev):
    """The scenario, assertions and tolerances of test_graph_gpu.py::test_whole_step_graph_matches_eager (amp leg) on the fp16 ResNet
    fixture: bench.py's GraphStep replays what the eager step computes.  Both sides differentiate the GradScaler's scaled loss at the
    initial scale 64 (the protocol of that file's fp16 Swin leg: GraphStep.INIT_SCALE), so the scaled gradients are compared."""
    _paths()
    import copy
    import bench
    from ocpg_amd.util.misc import NestedTensor
    amp = H16
    meta, args, model, crit = _tiny(dev)
    init_before, bench.GraphStep.INIT_SCALE = bench.GraphStep.INIT_SCALE, 64.0
    det_before = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        x, mask, targets, text = _tiny_batch(meta, dev)
        make_samples = lambda: NestedTensor(x.clone(), mask.clone())      # noqa: E731
        twin, twin_crit = copy.deepcopy(model), copy.deepcopy(crit)
        n_steps = 4

        def eager_losses(m, c):
            opt = bench.make_optimizer(m, args, fused=False)
            c.iter = 0
            step = bench.EagerStep(m, m, c, opt, make_samples, text, targets, args, amp)
            step.scaler = torch.amp.GradScaler("cuda", init_scale=64.0)
            return [float(step()) for _ in range(n_steps)]
        scaler = torch.amp.GradScaler("cuda", init_scale=64.0)
        twin_crit.iter = 0
        bench.forward_backward(twin, twin_crit, make_samples(), text, targets, amp, scaler=scaler)
        g_want = {k: p.grad.clone() for k, p in twin.named_parameters() if p.grad is not None}
        assert all(torch.isfinite(g_).all() for g_ in g_want.values())
        twin.zero_grad(set_to_none=True)
        twin_crit.iter = 0
        bench.forward_backward(twin, twin_crit, make_samples(), text, targets, amp, scaler=scaler)
        noise = {k: (p.grad - g_want[k]).abs().max().item() for k, p in twin.named_parameters() if p.grad is not None}
        twin.zero_grad(set_to_none=True)
        want = eager_losses(twin, twin_crit)
        crit.iter = 0
        opt = bench.make_optimizer(model, args, fused=False)
        step = bench.GraphStep(model, crit, opt, make_samples, text, targets, args, amp, 1)
        assert step.memset_nodes_replaced > 0
        for rep in range(2):                                    # two replays at the SAME parameters: identical to eager both times
            step.graph.replay()
            torch.cuda.synchronize()
            print(f"fp16 ResNet graph replay {rep}: loss {float(step.loss):.6f}, eager {want[0]:.6f}")
            assert abs(float(step.loss) - want[0]) <= 2e-3 * abs(want[0]), (rep, float(step.loss), want[0])
            for k, p in model.named_parameters():
                if k in g_want:
                    d = (p.grad - g_want[k]).abs().max().item()
                    assert d <= 8 * noise[k] + 0.15 * g_want[k].abs().max().item() + 1e-7, (rep, k, d, noise[k])
        got = [float(step()) for _ in range(n_steps)]
        print(f"fp16 ResNet graph steps {got}, eager {want}")
        tol = 3e-2
        for i, (a, b) in enumerate(zip(got, want)):
            assert a == a and abs(a - b) <= tol * (1 if i < 3 else 3) * abs(b), (i, got, want)
    finally:
        torch.backends.cudnn.deterministic = det_before
        bench.GraphStep.INIT_SCALE = init_before
