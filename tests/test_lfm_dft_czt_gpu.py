"""csrc/lfm_dft_czt.hip (both LFM transforms with a chirp-z line transform on one or both axes) through lfm_spectrum / lfm_inverse with
explicit chirp axes, and through the block.

The protocol, the truth (torch.fft in fp64 on the same inputs, on the host) and the FORM of the bound are those of
tests/test_lfm_dft_any_gpu.py: a 2-D transform errs, in every element, by at most 3 (S_h + S_w) u sum_map |input| (u = 2^-24), plus the
gate / norm / store terms written there (K_FWD = 3 (S_h + S_w) + 3, K_INV = 3 (S_h + S_w) + 6, the 16-bit store, gcoef's 3e-5 |ref| + 1e-6).
An axis that is not a chirp axis keeps its S = the sum of (R + 2) over its plan's stages.  A chirp axis is held to TWO values of S:

(a) derived for the kernel's structure.  A chirp line is X_k = c_k IFFT_M(FFT_M(a) B)_k, M = 256, a_n = x_n c_n.  Both M-point transforms are
    two radix-16 stages, each built from two levels of radix-4 butterflies: four levels each, S_M = 4 (4 + 2) = 24, so by the stage model
    of that file an M-point transform errs by at most 3 S_M u times the sum of the moduli of its inputs (the constant W_16 factors between
    the levels and the W_256 factors between the stages are the "+ 2" of a level).  In units of u sum_line |x|, for output k:
      * a_n: one complex product with a rounded factor, <= 4 |x_n|; it passes the forward transform with weight 1 into every A_k: 4;
      * the forward transform on inputs that sum to at most sum |x|: 3 S_M in every A_k;
      * both reach the result through B_k and the inverse transform, sum_k |B_k| / M = beta (the table holds B / M, so beta is the SUM of the
        moduli of the table's B entries, the mean of |B_k|): (3 S_M + 4) beta;
      * the product with B (rounded factor): 4 |A_k B_k| / M summed over k, <= 4 beta;
      * the inverse transform on inputs |A_k B_k| / M that sum to at most beta sum |x| (the division by M is exact, folded into the table):
        3 S_M beta;
      * the product with c_k: 4 |y_k|, |y_k| = |X_k| <= sum |x|: 4; and the rounded chirp in a_n and c_k, u each, is inside the 4s.
    Together (6 S_M + 8) beta + 8 = 3 S, S = ((6 S_M + 8) beta + 8) / 3 -- about 50 beta; beta is 10.2 at L = 65, 13.1 at 107, 14.4 at 127.
(b) S = L + 2: what tests/test_lfm_dft_any_gpu.py demands of the direct stage for that length, the route this one replaces.
Both are asserted.  Reported and not asserted: max error over torch.fft-fp32's (both torch.fft runs are on the host).
"""
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24
U16 = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
S_M = 24
# (n, c, h, w), chirp axes (h, w)
SHAPES = [((2, 36, 6, 107), (False, True)), ((1, 70, 83, 5), (True, False)), ((1, 8, 128, 65), (True, True)), ((1, 33, 4, 127), (False, True))]
CASES = [(s, a, torch.float32) for s, a in SHAPES] + [(*SHAPES[0], torch.bfloat16), (*SHAPES[0], torch.float16)]
NAMES = {"ocpg_lfm_spectrum_fwd_czt": 1, "ocpg_lfm_spectrum_inv_czt": 1}


def _s_plan(n):
    from ocpg_amd.models.ops.functions import spectral_func as sf
    return sum(r + 2 for r in sf._axis_plan(n) if r != 1)


def _s_derived(n):
    """(a): from the fp64 table of the length"""
    from ocpg_amd.models.ops.functions import spectral_func as sf
    t = torch.view_as_complex(sf._twiddles_czt(n, "cpu").double().contiguous())
    beta = max(t[128:384].abs().sum().item(), t[384:640].abs().sum().item())
    return ((6 * S_M + 8) * beta + 8) / 3


def _s_both(shape, axes):
    """S_h + S_w under (a) and under (b)"""
    _, _, h, w = shape
    a = sum(_s_derived(n) if on else _s_plan(n) for n, on in zip((h, w), axes))
    b = sum(n + 2 if on else _s_plan(n) for n, on in zip((h, w), axes))
    return {"derived": a, "direct": b}


def _store(truth, bound, dt):
    """+ the rounding of a result stored in dt"""
    if dt == torch.float32:
        return bound
    return bound + U16[dt] * (truth.abs() + bound) + (2.0 ** -24 if dt == torch.float16 else 0.0)


def _cabs(t, c):
    return torch.complex(t[:, :c].double(), t[:, c:].double()).abs()


def _report(name, shape, dt, err, lib_err, ratios):
    print(f"lfm_dft_czt {name} {shape} {str(dt)[6:]}: max err {err:.3e}  torch.fft-fp32 {lib_err:.3e}  ratio {err / max(lib_err, 1e-30):.2f}  "
          + "  ".join(f"err/bound({k}) {v:.5f}" for k, v in ratios.items()))


def _check(name, shape, dt, got, truth, lib32, bounds):
    """bounds: {which: elementwise bound}; prints every figure, then asserts every bound"""
    err = (got.double() - truth).abs()
    ratios = {k: (err / b).max().item() for k, b in bounds.items()}
    _report(name, shape, dt, err.max().item(), (lib32.double() - truth).abs().max().item(), ratios)
    for k, b in bounds.items():
        assert (err <= b).all(), (name, k, ratios[k])


@pytest.mark.parametrize("shape,axes,dt", CASES, ids=[f"{'x'.join(map(str, s))}-{'hw'[a[1]] if sum(a) == 1 else 'both'}-{str(d)[6:]}" for s, a, d in CASES])
def test_kernels_against_fp64(dev, shape, axes, dt):
    from ocpg_amd import _lib
    from ocpg_amd.models.ops.functions import spectral_func as sf
    n, c, h, w = shape
    torch.manual_seed(h * 131 + w)
    ss = _s_both(shape, axes)
    k_fwd = {k: 3 * v + 3 for k, v in ss.items()}
    k_inv = {k: 3 * v + 6 for k, v in ss.items()}

    def q(t):              # a 16-bit pass INPUT is made exactly representable
        return t.to(dt).float()
    x = torch.randn(n, c, h, w, device=dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    coef = torch.rand(n, device=dev).requires_grad_(True)
    high = torch.rand(h, w, device=dev)
    go = q(torch.randn(n, 2 * c, h, w, device=dev))
    calls = _lib.census(True)
    z = sf.lfm_spectrum(x, coef, high, dt, axes)
    gx, gcoef = torch.autograd.grad((z.float() * go).sum(), (x, coef))
    _lib.census(False)
    assert calls == NAMES, calls
    assert z.shape == (n, 2 * c, h, w) and z.dtype == dt and z.permute(0, 2, 3, 1).is_contiguous()
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
    _check("z", shape, dt, z, zt, z32.detach(), {k: _store(zt, (gate.abs() * (kf * U32) * sum_x).repeat(1, 2, 1, 1), dt) for k, kf in k_fwd.items()})
    # gx = Re(inverse of gate * go), norm 1
    sum_g = (_cabs(go, c) * gate.abs()).sum((2, 3), keepdim=True)
    _check("gx", shape, dt, gx, gxt, gx32, {k: ((ki * U32) * sum_g).expand_as(gxt) for k, ki in k_inv.items()})
    # gcoef
    terms = (hd * (go[:, :c].double() * spec.real).abs() + hd * (go[:, c:].double() * spec.imag).abs()).sum((1, 2, 3))
    bgc = 3e-5 * gct.abs() + 1e-6 + U16[dt] * (1 + 2.0 ** -6) * terms
    egc = (gcoef.double() - gct).abs()
    print(f"lfm_dft_czt gcoef {shape} {str(dt)[6:]}: max err {egc.max().item():.3e}  torch.fft-fp32 {(gc32.double() - gct).abs().max().item():.3e}  "
          f"err / (3e-5 |ref| + 1e-6) = {(egc / (3e-5 * gct.abs() + 1e-6)).max().item():.3f}")
    assert (egc <= bgc).all(), ("gcoef", (egc / bgc).max().item())
    # x + ifft2(.).real and its gradients
    y = q(torch.randn(n, 2 * c, h, w, device=dev)).to(dt).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    gr = torch.randn(n, c, h, w, device=dev)
    calls = _lib.census(True)
    r = sf.lfm_inverse(y, x, axes)
    gy, gxr = torch.autograd.grad((r * gr).sum(), (y, x))
    _lib.census(False)
    assert torch.equal(gxr, gr)
    assert calls == NAMES, calls
    assert r.dtype == torch.float32 and r.permute(0, 2, 3, 1).is_contiguous() and gy.dtype == dt
    r, gy, gr, y = r.detach().cpu(), gy.cpu(), gr.cpu(), y.detach().cpu()
    yd = y.double().requires_grad_(True)
    rt = xd.detach() + torch.fft.ifft2(torch.complex(yd[:, :c], yd[:, c:]), s=(h, w)).real
    gyt, = torch.autograd.grad((rt * gr.double()).sum(), yd)
    rt = rt.detach()
    y32 = y.float()
    r32 = xc + torch.fft.ifft2(torch.complex(y32[:, :c], y32[:, c:]), s=(h, w)).real
    sum_y = _cabs(y, c).sum((2, 3), keepdim=True)
    _check("x+ifft2", shape, dt, r, rt, r32, {k: (ki * U32 / (h * w)) * sum_y + U32 * xc.double().abs() for k, ki in k_inv.items()})
    # gy = fft2(g) / hw as a pair, no gate: the call with coef and high absent
    sum_r = gr.double().abs().sum((2, 3), keepdim=True)
    g32 = torch.fft.fft2(gr, norm="forward")
    _check("gy", shape, dt, gy, gyt, torch.cat([g32.real, g32.imag], 1),
           {k: _store(gyt, ((kf * U32 / (h * w)) * sum_r).expand(n, c, h, w).repeat(1, 2, 1, 1), dt) for k, kf in k_fwd.items()})


def test_chirp_against_direct_stage(dev):
    """(2, 36, 6, 107) through the direct stage of csrc/lfm_dft_any.hip (no chirp axis) and through the chirp axis: both inside the bound
    of the direct stage, (b); their distance is printed."""
    from ocpg_amd import _lib
    from ocpg_amd.models.ops.functions import spectral_func as sf
    shape, axes = SHAPES[0]
    n, c, h, w = shape
    torch.manual_seed(11)
    kf, ki = 3 * _s_both(shape, axes)["direct"] + 3, 3 * _s_both(shape, axes)["direct"] + 6
    x = torch.randn(n, c, h, w, device=dev).contiguous(memory_format=torch.channels_last)
    coef, high = torch.rand(n, device=dev), torch.rand(h, w, device=dev)
    y = torch.randn(n, 2 * c, h, w, device=dev).contiguous(memory_format=torch.channels_last)
    got = {}
    for name, ax in (("direct", (False, False)), ("chirp", axes)):
        calls = _lib.census(True)
        got[name] = (sf.lfm_spectrum(x, coef, high, torch.float32, ax).cpu(), sf.lfm_inverse(y, x, ax).cpu())
        _lib.census(False)
        assert set(calls) == ({"ocpg_lfm_spectrum_fwd_any", "ocpg_lfm_spectrum_inv_any"} if name == "direct" else set(NAMES)), calls
    xd, yd = x.cpu().double(), y.cpu().double()
    gate = 1 - coef.cpu().double().view(n, 1, 1, 1) * high.cpu().double()
    spec = torch.fft.fft2(xd) * gate
    zt = torch.cat([spec.real, spec.imag], 1)
    rt = xd + torch.fft.ifft2(torch.complex(yd[:, :c], yd[:, c:]), s=(h, w)).real
    bz = (gate.abs() * (kf * U32) * xd.abs().sum((2, 3), keepdim=True)).repeat(1, 2, 1, 1)
    br = (ki * U32 / (h * w)) * _cabs(y.cpu(), c).sum((2, 3), keepdim=True) + U32 * xd.abs()
    for name, (z, r) in got.items():
        ez, er = (z.double() - zt).abs(), (r.double() - rt).abs()
        print(f"lfm_dft_czt {name}: z err/bound {(ez / bz).max().item():.5f} (max {ez.max().item():.3e})  x+ifft2 err/bound {(er / br).max().item():.5f}")
        assert (ez <= bz).all() and (er <= br).all(), name
    dz, dr = (got["chirp"][0] - got["direct"][0]).abs(), (got["chirp"][1] - got["direct"][1]).abs()
    print(f"lfm_dft_czt chirp - direct: z max {dz.max().item():.3e} (over bound {(dz.double() / bz).max().item():.5f})  x+ifft2 max {dr.max().item():.3e}")


def test_refusals_write_nothing(dev):
    """A chirp axis of 64 and of 129: -2000 from both entries, outputs untouched."""
    from ocpg_amd._lib import lib
    st = torch.cuda.current_stream().cuda_stream
    tw = torch.zeros(4096, device=dev)
    for h, w, hp, wp, on in ((4, 64, (1, 4, 1), (1, 1, 64), (False, True)), (4, 129, (1, 4, 1), (1, 1, 129), (False, True)),
                             (64, 4, (1, 1, 64), (1, 4, 1), (True, False)), (129, 4, (1, 1, 129), (1, 4, 1), (True, False))):
        n, c = 1, 8
        x = torch.randn(n, h, w, c, device=dev)
        tmp = torch.full((n, h, w // 2 + 1, c, 2), 7.0, device=dev)
        pair = torch.full((n, h, w, 2 * c), 7.0, device=dev)
        out = torch.full((n, h, w, c), 7.0, device=dev)
        cz = [tw.data_ptr() if o else None for o in on]
        assert lib().ocpg_lfm_spectrum_fwd_czt(x.data_ptr(), None, None, n, h, w, c, tw.data_ptr(), tw.data_ptr(), 1.0, tmp.data_ptr(), pair.data_ptr(), 0,
                                               *hp, *wp, *cz, st) == -2000
        assert lib().ocpg_lfm_spectrum_inv_czt(pair.data_ptr(), 0, None, None, None, None, n, h, w, c, tw.data_ptr(), tw.data_ptr(), 1.0, tmp.data_ptr(),
                                               None, out.data_ptr(), *hp, *wp, *cz, st) == -2000
        torch.cuda.synchronize()
        assert (tmp == 7).all() and (pair == 7).all() and (out == 7).all()


@pytest.mark.parametrize("amp", [None, torch.bfloat16])
def test_block_routing_and_switch(dev, amp, monkeypatch):
    """LFMResizeAdaptive on a 6 x 107 map (csrc/lfm_dft_czt.hip, chirp along w) chained into a 3 x 54 one (csrc/lfm_dft.hip), under
    OCPG_STRICT_HIP=1: the census names the entry points, nothing is counted as a fallback, and output / input gradients / every parameter
    gradient equal the run with the switch off (rocFFT for the first map, one counted fallback per forward, an error under strict mode) at
    the bounds of test_block_routing_and_switch in tests/test_lfm_dft_any_gpu.py."""
    from ocpg_amd import _lib
    from ocpg_amd.models import fallbacks, modules
    monkeypatch.setattr(modules, "DFT_CL", True)
    monkeypatch.setattr(modules, "DFT_ANY", True)
    monkeypatch.setattr(modules, "DFT_CZT_FORCE", False)
    monkeypatch.setattr(modules, "DFT_CZT_MIN_PRIME", 83)
    torch.manual_seed(1)
    lfm = modules.LFMResizeAdaptive(72, 7).to(dev)
    x1 = torch.randn(3, 72, 6, 107, device=dev).contiguous(memory_format=torch.channels_last)
    x2 = torch.randn(3, 72, 3, 54, device=dev)
    names = ("ocpg_lfm_spectrum_fwd_czt", "ocpg_lfm_spectrum_inv_czt", "ocpg_lfm_spectrum_fwd", "ocpg_lfm_spectrum_inv")

    def run(on, dtype):
        monkeypatch.setattr(modules, "DFT_CZT", on)
        if on:
            monkeypatch.setenv("OCPG_STRICT_HIP", "1")
        else:
            monkeypatch.delenv("OCPG_STRICT_HIP", raising=False)
        fallbacks.reset()
        a, b_ = x1.clone(memory_format=torch.preserve_format).requires_grad_(True), x2.clone().requires_grad_(True)
        lfm.zero_grad()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
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
        assert not any(k.endswith("_any") for k in calls), calls
        snap = {k: v for k, v in fallbacks.snapshot().items() if k.startswith("LFM")}
        assert (not snap) if on else (len(snap) == 1 and list(snap.values()) == [1]), snap
        return [y1.detach().float(), y2.detach().float(), a.grad, b_.grad] + [p.grad.clone() for p in lfm.parameters()]
    try:
        if amp is None:
            for u, v in zip(run(True, None), run(False, None)):
                assert (u - v).abs().max().item() <= 3e-5 * v.abs().max().item() + 1e-7, ((u - v).abs().max().item(), v.abs().max().item())
            # with the switch off the first map raises under strict mode
            monkeypatch.setattr(modules, "DFT_CZT", False)
            monkeypatch.setenv("OCPG_STRICT_HIP", "1")
            with pytest.raises(RuntimeError, match="LFM"):
                lfm(x1)
        else:
            ref, lib_, own = run(False, None), run(False, amp), run(True, amp)
            for r, a, b_ in zip(ref, lib_, own):
                scale = r.abs().max().item()
                assert (b_ - r).abs().max().item() <= 1.5 * (a - r).abs().max().item() + 1e-2 * scale + 1e-7, \
                    ((b_ - r).abs().max().item(), (a - r).abs().max().item(), scale)
    finally:
        fallbacks.reset()


def test_graph_replay_is_bitwise_eager(dev):
    """Both entry points captured once on (2, 36, 6, 107), chirp along w, and replayed: bit for bit the eager results."""
    from ocpg_amd.models.ops.functions import spectral_func as sf
    (n, c, h, w), axes = SHAPES[0]
    torch.manual_seed(5)
    x = torch.randn(n, h, w, c, device=dev)
    coef, high = torch.rand(n, device=dev), torch.rand(h, w, device=dev)
    g = torch.randn(n, h, w, 2 * c, device=dev)

    def step():
        pair = sf._spectrum(x, coef, high, 1.0, torch.float32, axes)
        out, part = sf._inverse(g, coef, high, pair, True, 1.0 / (h * w), x, axes)
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
