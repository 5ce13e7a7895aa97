"""csrc/lfm_dft_any.hip (both LFM transforms for every map size up to 256 x 256) through lfm_spectrum / lfm_inverse and through the block.

The truth is torch.fft in fp64 on the same fp32 (or 16-bit) inputs.  THE BOUND is a-priori, elementwise, and not tuned to the kernels:

A stage of radix R forms every output as a sum of R complex products with fp32-rounded twiddles.  With u = 2^-24 (fp32 unit roundoff):
each component of an output is a chain of 2 R fused multiply-adds, so its error is at most 2 R u sum_j |x_j| (|x_re w_re| + |x_im w_im|
<= |x||w| = |x|), the complex error sqrt(2) times that; the rounded twiddles add u sum_j |x_j|; the twiddle between stages (one complex
product with a rounded factor) adds at most 4 u |y| <= 4 u sum_j |x_j|.  Together <= (2 sqrt(2) R + 5) u sum |x_j| <= 3 (R + 2) u sum |x_j|.
Later stages have unit-modulus weights, so a stage's error reaches a final output with weight <= 1, and a stage's inputs sum to at most the
line's: to first order a LINE transform errs by at most 3 S u sum_line |x|, S = the sum over the plan's stages that are not 1 of (R + 2).
The second pass adds its own error on inputs that sum to at most the map's and carries the first pass's error with weight 1 per element:
a 2-D transform errs, in every element, by at most 3 (S_h + S_w) u sum_map |input| (the direct prime stage is the case R = p).
  * forward z = norm * gate * fft2(x): the gate (one fma), norm and the product are three roundings of z: + 3 u |z|, |z| <= |norm gate| sum|x|:
        |dz[n, c, u, v]| <= |norm gate[n, u, v]| (3 (S_h + S_w) + 3) u sum_hw |x[n, c]|            (K_FWD)
  * inverse out = norm * Re(inverse(Herm(gate * Y))) + residual: the Hermitian part's prologue rounds a ga, b gb, their sum (3 u of an input
    whose modulus is at most (|a||ga| + |b||gb|) / 2; over the plane those sum to at most sum |Y||gate|), norm and the residual add round twice:
        |dout| <= norm (3 (S_h + S_w) + 6) u sum_hw |Y_c[n, c]||gate[n]| + u |residual|              (K_INV)
  * a 16-bit pair is rounded once on the way out: + u16 (|truth| + bound), u16 = 2^-8 (bf16) / 2^-11 (fp16, + 2^-24 below its normal range);
    16-bit INPUTS of the passes are made exactly representable here, so they add nothing.
  * gcoef: the project's bound for this quantity, 3e-5 |ref| + 1e-6 (tests/test_model_gpu.py, test_lfm_dft_kernels_equal_torch_fft); with a
    16-bit pair the saved spectrum z has a relative error u16 per component, so + u16 sum high (|g_re S_re| + |g_im S_im|) (1 + 2^-6 for the
    second-order term).
The backward passes are the same two kernels (gx = inverse(gate * gz), norm 1; gy = forward(g), norm 1 / hw, coef / high absent -- the
call LFMInverse.backward makes), so the same forms apply to THEIR inputs.  Reported and not asserted: max error over torch.fft-fp32's
(both torch.fft runs are on the host: a GPU FFT plan per size would cost seconds).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24
U16 = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
SHAPES = [(2, 36, 23, 37), (1, 70, 17, 34), (2, 8, 51, 1), (1, 130, 6, 125), (1, 5, 127, 3), (1, 66, 129, 2), (1, 33, 4, 251), (1, 40, 250, 19),
          (1, 64, 256, 255), (2, 36, 8, 34)]
CASES = [(s, torch.float32) for s in SHAPES] + [(SHAPES[0], torch.bfloat16), (SHAPES[0], torch.float16)]


def _s(n):
    from ocpg_amd.models.ops.functions import spectral_func as sf
    return sum(r + 2 for r in sf._axis_plan(n) if r != 1)


def _store(truth, bound, dt):
    """+ the rounding of a result stored in dt"""
    if dt == torch.float32:
        return bound
    return bound + U16[dt] * (truth.abs() + bound) + (2.0 ** -24 if dt == torch.float16 else 0.0)


def _cabs(t, c):
    return torch.complex(t[:, :c].double(), t[:, c:].double()).abs()


def _report(name, shape, dt, err, lib_err):
    print(f"lfm_dft_any {name} {shape} {str(dt)[6:]}: max err {err:.3e}  torch.fft-fp32 {lib_err:.3e}  ratio {err / max(lib_err, 1e-30):.2f}")


@pytest.mark.parametrize("shape,dt", CASES, ids=[f"{'x'.join(map(str, s))}-{str(d)[6:]}" for s, d in CASES])
def test_kernels_against_fp64(dev, shape, dt):
    from ocpg_amd import _lib
    from ocpg_amd.models.ops.functions import spectral_func as sf
    n, c, h, w = shape
    torch.manual_seed(h * 131 + w)
    assert not sf.dft_supported(h, w) and sf.dft_any_supported(h, w)
    k_fwd, k_inv = 3 * (_s(h) + _s(w)) + 3, 3 * (_s(h) + _s(w)) + 6

    def q(t):              # a 16-bit pass INPUT is made exactly representable
        return t.to(dt).float()
    x = torch.randn(n, c, h, w, device=dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    coef = torch.rand(n, device=dev).requires_grad_(True)
    high = torch.rand(h, w, device=dev)
    go = q(torch.randn(n, 2 * c, h, w, device=dev))
    calls = _lib.census(True)
    z = sf.lfm_spectrum(x, coef, high, dt)
    gx, gcoef = torch.autograd.grad((z.float() * go).sum(), (x, coef))
    _lib.census(False)
    assert calls == {"ocpg_lfm_spectrum_fwd_any": 1, "ocpg_lfm_spectrum_inv_any": 1}, calls
    assert z.shape == (n, 2 * c, h, w) and z.dtype == dt and z.permute(0, 2, 3, 1).is_contiguous()
    # the truth, fp64, and the library's fp32 on the same tensors, both on the host (no FFT plans are built on the GPU for these sizes)
    z, gx, gcoef, go = z.detach().cpu(), gx.cpu(), gcoef.cpu(), go.cpu()
    xc, cc, high = x.detach().cpu(), coef.detach().cpu(), high.cpu()
    xd, cd, hd = xc.double().requires_grad_(True), cc.double().requires_grad_(True), high.double()
    gate = 1 - cd.view(n, 1, 1, 1) * hd
    spec = torch.fft.fft2(xd)
    zt = torch.cat([(spec * gate).real, (spec * gate).imag], 1)
    gxt, gct = torch.autograd.grad((zt * go.double()).sum(), (xd, cd))
    gate, spec, zt = gate.detach(), spec.detach(), zt.detach()
    sum_x = xc.double().abs().sum((2, 3), keepdim=True)
    x32, c32 = xc.clone().requires_grad_(True), cc.clone().requires_grad_(True)
    s32 = torch.fft.fft2(x32) * (1 - c32.view(n, 1, 1, 1) * high)
    z32 = torch.cat([s32.real, s32.imag], 1)
    gx32, gc32 = torch.autograd.grad((z32 * go).sum(), (x32, c32))
    # z
    bz = _store(zt, (gate.abs() * (k_fwd * U32) * sum_x).repeat(1, 2, 1, 1), dt)
    ez = (z.double() - zt).abs()
    _report("z", shape, dt, ez.max().item(), (z32.detach().double() - zt).abs().max().item())
    assert (ez <= bz).all(), ("z", (ez / bz).max().item())
    # gx = Re(inverse of gate * go), norm 1
    bgx = (k_inv * U32) * (_cabs(go, c) * gate.abs()).sum((2, 3), keepdim=True)
    egx = (gx.double() - gxt).abs()
    _report("gx", shape, dt, egx.max().item(), (gx32.double() - gxt).abs().max().item())
    assert (egx <= bgx).all(), ("gx", (egx / bgx).max().item())
    # gcoef
    terms = (hd * (go[:, :c].double() * spec.real).abs() + hd * (go[:, c:].double() * spec.imag).abs()).sum((1, 2, 3))
    bgc = 3e-5 * gct.abs() + 1e-6 + U16[dt] * (1 + 2.0 ** -6) * terms
    egc = (gcoef.double() - gct).abs()
    _report("gcoef", shape, dt, egc.max().item(), (gc32.double() - gct).abs().max().item())
    print(f"lfm_dft_any gcoef {shape}: err / (3e-5 |ref| + 1e-6) = {(egc / (3e-5 * gct.abs() + 1e-6)).max().item():.3f}, "
          f"library err / same = {((gc32.double() - gct).abs() / (3e-5 * gct.abs() + 1e-6)).max().item():.3f}")
    assert (egc <= bgc).all(), ("gcoef", (egc / bgc).max().item())
    # x + ifft2(.).real and its gradients
    y = q(torch.randn(n, 2 * c, h, w, device=dev)).to(dt).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    gr = torch.randn(n, c, h, w, device=dev)
    calls = _lib.census(True)
    r = sf.lfm_inverse(y, x)
    gy, gxr = torch.autograd.grad((r * gr).sum(), (y, x))
    _lib.census(False)
    assert torch.equal(gxr, gr)
    assert calls == {"ocpg_lfm_spectrum_fwd_any": 1, "ocpg_lfm_spectrum_inv_any": 1}, calls
    assert r.dtype == torch.float32 and r.permute(0, 2, 3, 1).is_contiguous() and gy.dtype == dt
    r, gy, gr, y = r.detach().cpu(), gy.cpu(), gr.cpu(), y.detach().cpu()
    yd = y.double().requires_grad_(True)
    rt = xd.detach() + torch.fft.ifft2(torch.complex(yd[:, :c], yd[:, c:]), s=(h, w)).real
    gyt, = torch.autograd.grad((rt * gr.double()).sum(), yd)
    rt = rt.detach()
    y32 = y.float()
    r32 = xc + torch.fft.ifft2(torch.complex(y32[:, :c], y32[:, c:]), s=(h, w)).real
    br = (k_inv * U32 / (h * w)) * _cabs(y, c).sum((2, 3), keepdim=True) + U32 * xc.double().abs()
    er = (r.double() - rt).abs()
    _report("x+ifft2", shape, dt, er.max().item(), (r32.double() - rt).abs().max().item())
    assert (er <= br).all(), ("r", (er / br).max().item())
    # gy = fft2(g) / hw as a pair, no gate: the call with coef and high absent
    bgy = _store(gyt, ((k_fwd * U32 / (h * w)) * gr.double().abs().sum((2, 3), keepdim=True)).expand(n, c, h, w).repeat(1, 2, 1, 1), dt)
    egy = (gy.double() - gyt).abs()
    g32 = torch.fft.fft2(gr, norm="forward")
    _report("gy", shape, dt, egy.max().item(), (torch.cat([g32.real, g32.imag], 1).double() - gyt).abs().max().item())
    assert (egy <= bgy).all(), ("gy", (egy / bgy).max().item())


def test_refusals_write_nothing(dev):
    """Both new entries answer -2000 for H = 257 and leave their outputs alone; the old entries still refuse 23 x 37."""
    from ocpg_amd._lib import lib
    n, c, h, w = 1, 8, 257, 4
    st = torch.cuda.current_stream().cuda_stream
    x = torch.randn(n, h, w, c, device=dev)
    tw = torch.zeros(4096, device=dev)
    tmp = torch.full((n, h, w // 2 + 1, c, 2), 7.0, device=dev)
    pair = torch.full((n, h, w, 2 * c), 7.0, device=dev)
    out = torch.full((n, h, w, c), 7.0, device=dev)
    for plan in ((1, 1, 257), (1, 16, 16), (1, 1, 1)):
        assert lib().ocpg_lfm_spectrum_fwd_any(x.data_ptr(), None, None, n, h, w, c, tw.data_ptr(), tw.data_ptr(), 1.0, tmp.data_ptr(), pair.data_ptr(), 0,
                                               *plan, 1, 2, 2, st) == -2000
        assert lib().ocpg_lfm_spectrum_inv_any(pair.data_ptr(), 0, None, None, None, None, n, h, w, c, tw.data_ptr(), tw.data_ptr(), 1.0, tmp.data_ptr(),
                                               None, out.data_ptr(), *plan, 1, 2, 2, st) == -2000
    torch.cuda.synchronize()
    assert (tmp == 7).all() and (pair == 7).all() and (out == 7).all()
    h, w = 23, 37
    assert lib().ocpg_lfm_spectrum_fwd(x.data_ptr(), None, None, 1, h, w, 1, tw.data_ptr(), tw.data_ptr(), 1.0, tmp.data_ptr(), pair.data_ptr(), 0, st) == -2000
    assert lib().ocpg_lfm_spectrum_inv(pair.data_ptr(), 0, None, None, None, None, 1, h, w, 1, tw.data_ptr(), tw.data_ptr(), 1.0, tmp.data_ptr(), None,
                                       out.data_ptr(), st) == -2000
    torch.cuda.synchronize()
    assert (tmp == 7).all() and (pair == 7).all() and (out == 7).all()


@pytest.mark.parametrize("amp", [None, torch.bfloat16])
def test_block_routing_and_switch(dev, amp, monkeypatch):
    """LFMResizeAdaptive on a 23 x 40 map (csrc/lfm_dft_any.hip) chained into a 12 x 20 one (csrc/lfm_dft.hip): the census names the entry
    points, nothing is counted as a fallback, and output / input gradients / every parameter gradient equal the run with the switch off
    (rocFFT for the first map) at the bound of test_lfm_block_own_transforms_equal_library_fft."""
    from ocpg_amd import _lib
    from ocpg_amd.models import fallbacks, modules
    monkeypatch.delenv("OCPG_STRICT_HIP", raising=False)
    torch.manual_seed(1)
    lfm = modules.LFMResizeAdaptive(72, 7).to(dev)
    x1 = torch.randn(3, 72, 23, 40, device=dev).contiguous(memory_format=torch.channels_last)
    x2 = torch.randn(3, 72, 12, 20, device=dev)
    names = ("ocpg_lfm_spectrum_fwd_any", "ocpg_lfm_spectrum_inv_any", "ocpg_lfm_spectrum_fwd", "ocpg_lfm_spectrum_inv")

    def run(on, dtype):
        monkeypatch.setattr(modules, "DFT_ANY", on)
        fallbacks.reset()
        a, b_ = x1.clone(memory_format=torch.preserve_format).requires_grad_(True), x2.clone().requires_grad_(True)
        lfm.zero_grad()
        with torch.autocast("cuda", dtype=dtype, enabled=dtype is not None):
            calls = _lib.census(True)
            y1, g = lfm(a)
            first = tuple(calls.get(k, 0) for k in names)
            y2, _ = lfm(b_, g)
            fwd = tuple(calls.get(k, 0) for k in names)
        (y1.float().square().mean() + y2.float().square().mean()).backward()
        _lib.census(False)
        assert first == ((1, 1, 0, 0) if on else (0, 0, 0, 0)) and fwd == ((1, 1, 1, 1) if on else (0, 0, 1, 1)), (first, fwd)
        assert tuple(calls.get(k, 0) for k in names) == ((2, 2, 2, 2) if on else (0, 0, 2, 2)), calls
        assert not any(k.startswith("LFM") for k in fallbacks.snapshot()), fallbacks.snapshot()
        return [y1.detach().float(), y2.detach().float(), a.grad, b_.grad] + [p.grad.clone() for p in lfm.parameters()]
    if amp is None:
        for u, v in zip(run(True, None), run(False, None)):
            assert (u - v).abs().max().item() <= 3e-5 * v.abs().max().item() + 1e-7, ((u - v).abs().max().item(), v.abs().max().item())
    else:
        ref, lib_, own = run(False, None), run(False, amp), run(True, amp)
        for r, a, b_ in zip(ref, lib_, own):
            scale = r.abs().max().item()
            assert (b_ - r).abs().max().item() <= 1.5 * (a - r).abs().max().item() + 1e-2 * scale + 1e-7, \
                ((b_ - r).abs().max().item(), (a - r).abs().max().item(), scale)


def test_longer_lines_are_a_counted_fallback(dev, monkeypatch):
    """A 4 x 300 map is past what either kernel file serves: with the switch on the library route is counted once per forward and is an
    error under OCPG_STRICT_HIP=1; with the switch off it is the parent's silent route."""
    from ocpg_amd.models import fallbacks, modules
    torch.manual_seed(2)
    lfm = modules.LFMResizeAdaptive(8, 7).to(dev)
    x = torch.randn(2, 8, 4, 300, device=dev)
    monkeypatch.delenv("OCPG_STRICT_HIP", raising=False)
    monkeypatch.setattr(modules, "DFT_ANY", True)
    fallbacks.reset()
    try:
        with pytest.warns(RuntimeWarning):
            y, _ = lfm(x)
        snap = {k: v for k, v in fallbacks.snapshot().items() if k.startswith("LFM")}
        assert len(snap) == 1 and list(snap.values()) == [1], snap
        monkeypatch.setattr(modules, "DFT_ANY", False)
        fallbacks.reset()
        y0, _ = lfm(x)
        assert not any(k.startswith("LFM") for k in fallbacks.snapshot()) and torch.equal(y, y0)
        monkeypatch.setattr(modules, "DFT_ANY", True)
        monkeypatch.setenv("OCPG_STRICT_HIP", "1")
        with pytest.raises(RuntimeError, match="LFM"):
            lfm(x)
    finally:
        fallbacks.reset()


def test_graph_replay_is_bitwise_eager(dev):
    """Both new entry points captured once on (2, 36, 23, 37) and replayed: bit for bit the eager results (sizes and plans travel by value,
    nothing is zeroed or accumulated)."""
    from ocpg_amd.models.ops.functions import spectral_func as sf
    n, c, h, w = 2, 36, 23, 37
    torch.manual_seed(5)
    x = torch.randn(n, h, w, c, device=dev)
    coef, high = torch.rand(n, device=dev), torch.rand(h, w, device=dev)
    g = torch.randn(n, h, w, 2 * c, device=dev)

    def step():
        pair = sf._spectrum(x, coef, high, 1.0, torch.float32)
        out, part = sf._inverse(g, coef, high, pair, True, 1.0 / (h * w), x)
        return pair, out, part

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = [t.clone() for t in step()]            # (also builds the tables: a host-to-device copy, before the capture)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        static = step()
    for t in static:
        t.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    for a, b_ in zip(static, eager):
        assert torch.equal(a, b_)
