"""The decoder / head / neck side of fp16 autocast (the reference's --amp mode) on own kernels: the fp16 instantiations of the few-row
Linear (csrc/small_linear.hip: sl_fwd_f16 / sl_bwd_f16 behind ocpg_small_linear_{fwd,bwd}_h16, dtype 2) and of the neck's split-K 3x3
convolution (conv3x3_mfma_f16<false, 64, true> behind ocpg_conv3x3_mfma_fwd_splitk_h16; input gradient by
ocpg_conv3x3_mfma_dgrad_w_h16 on the convolution's own weight), their gates and A/B switches, and a tiny training step with GradScaler.

Bounds.  fp16 has three more mantissa bits than bf16, so every bound is the bf16 test's bound times 2^-3 (the rule of
test_resnet_fp16_gpu.py's docstring):
  few-row Linear y, gx, gw, gb   max|a - b| <= 2^-10 max|b| + 1e-6     (test_model_gpu.py::test_small_linear_kernel: 2^-7, one bf16 ulp;
                                                                        both sides round the same fp32-accumulated sums once to fp16)
  split-K conv rel(y)            7.5e-4                                  (test_conv3x3_splitk_kernel: 6e-3)
  split-K conv rel(gx, gw, gb)   1.9e-3                                  (there: 1.5e-2)
  tiny step loss                 2e-2 relative of the fp32 run           (test_tiny_resnet_training_step_under_fp16_autocast)"""
import math

import pytest
import torch

from test_resnet_fp16_gpu import _paths, _ptr, _rel, _tiny, _tiny_batch

pytestmark = pytest.mark.gpu

H16 = torch.float16
BF16 = torch.bfloat16
CL = torch.channels_last


# ---- 1. the kernels against autocast's own path -----------------------------------------------------------------------------------
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("xdt", [torch.float32, H16])
@pytest.mark.parametrize("r,cin,cout,bias", [(50, 256, 256, True), (50, 256, 4, True), (200, 256, 4416, True), (10, 256, 1, False),
                                             (18, 256, 512, True), (50, 256, 384, True), (130, 128, 70, True), (1, 64, 64, True)])
def test_small_linear_fp16_kernel(dev, xdt, r, cin, cout, bias, relu):
    """The protocol and shapes of test_model_gpu.py::test_small_linear_kernel with fp16 operands under fp16 autocast: against F.linear
    (+ relu) on the library path with the same operands, y, gx (in x's dtype), gw, gb within 2^-10 max|ref| + 1e-6."""
    from ocpg_amd import _lib
    from ocpg_amd.models import amp_cache
    g = torch.Generator(device=dev).manual_seed(r * 131 + cout)
    x = torch.randn(2, r // 2 if r % 2 == 0 else r, cin, device=dev, generator=g).to(xdt)
    x = x if r % 2 == 0 else x[:1]
    w = (torch.randn(cout, cin, device=dev, generator=g) * cin ** -0.5).to(H16)
    b = torch.randn(cout, device=dev, generator=g).to(H16) if bias else None
    go = torch.randn(*x.shape[:-1], cout, device=dev, generator=g).to(H16)
    res = []
    for mine in (True, False):
        xi, wi = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
        bi = b.clone().requires_grad_(True) if bias else None
        calls = _lib.census(True)
        try:
            with torch.autocast("cuda", dtype=H16):
                if mine:
                    assert amp_cache._small_linear_ok(xi, wi, bi)
                    y = amp_cache.SmallLinearFunction.apply(xi, wi, bi, relu)
                else:
                    y = torch.nn.functional.linear(xi, wi, bi)
                    y = torch.relu(y) if relu else y
            assert y.dtype == H16
            grads = torch.autograd.grad((y.float() * go.float()).sum(), [xi, wi] + ([bi] if bias else []))
            torch.cuda.synchronize()
        finally:
            counts = dict(calls)
            _lib.census(False)
        if mine:
            assert counts == {"ocpg_small_linear_fwd_h16": 1, "ocpg_small_linear_bwd_h16": 1}, counts
        else:
            assert not [k for k in counts if "small_linear" in k], counts
        assert grads[0].dtype == xdt and grads[1].dtype == H16 and (not bias or grads[2].dtype == H16)
        res.append([y.float()] + [t.float() for t in grads])
    for name, a, b_ in zip(("y", "gx", "gw", "gb"), res[0], res[1]):
        err, ref = (a - b_).abs().max().item(), b_.abs().max().item()
        print(f"small_linear fp16 x={xdt} r{r} cin{cin} cout{cout} relu={relu} {name}: max|a - b| {err:.3e}, max|b| {ref:.3e}, bound {2 ** -10 * ref + 1e-6:.3e}")
        assert err <= 2 ** -10 * ref + 1e-6, (name, err, ref)


# ---- 2. the _h16 symbols: dtype 1 is the old kernel, other codes launch nothing ---------------------------------------------------
def test_small_linear_h16_with_dtype_1_is_the_old_symbol_and_bad_codes_launch_nothing(dev):
    from ocpg_amd._lib import lib, stream_ptr
    L, st = lib(), stream_ptr()
    r, cin, cout = 130, 128, 70
    g = torch.Generator(device=dev).manual_seed(11)
    x = torch.randn(r, cin, device=dev, generator=g)
    w = (torch.randn(cout, cin, device=dev, generator=g) * cin ** -0.5).to(BF16)
    b = torch.randn(cout, device=dev, generator=g).to(BF16)
    gy = torch.randn(r, cout, device=dev, generator=g)
    new = lambda dt, *s: torch.full(s, 7.0, dtype=dt, device=dev)      # noqa: E731
    y_a, y_b = new(BF16, r, cout), new(BF16, r, cout)
    assert L.ocpg_small_linear_fwd(_ptr(x), 1, _ptr(w), _ptr(b), r, cin, cout, 1, _ptr(y_a), st) == 0
    assert L.ocpg_small_linear_fwd_h16(_ptr(x), 1, _ptr(w), _ptr(b), r, cin, cout, 1, _ptr(y_b), 1, st) == 0
    out_a = [new(torch.float32, r, cin), new(BF16, cout, cin), new(BF16, cout)]
    out_b = [new(torch.float32, r, cin), new(BF16, cout, cin), new(BF16, cout)]
    assert L.ocpg_small_linear_bwd(_ptr(gy), 1, _ptr(x), 1, _ptr(w), _ptr(y_a), r, cin, cout, *[_ptr(t) for t in out_a], st) == 0
    assert L.ocpg_small_linear_bwd_h16(_ptr(gy), 1, _ptr(x), 1, _ptr(w), _ptr(y_a), r, cin, cout, *[_ptr(t) for t in out_b], 1, st) == 0
    torch.cuda.synchronize()
    assert torch.equal(y_a, y_b) and all(torch.equal(p, q) for p, q in zip(out_a, out_b))
    assert bool((y_a.float() != 7.0).any()) and all(bool((t.float() != 7.0).any()) for t in out_a)
    n, c, co, h, wd, stride = 1, 256, 64, 5, 5, 2
    sp = int(L.ocpg_conv3x3_mfma_splits(n, h, wd, c, co, stride))
    assert sp > 1
    m = n * 3 * 3
    xm, wm = torch.randn(n, h, wd, c, device=dev, generator=g).to(BF16), (torch.randn(co, 3, 3, c, device=dev, generator=g) * 0.02).to(BF16)
    bias = torch.randn(co, device=dev, generator=g)
    part = torch.empty(sp, m, co, device=dev)
    c_a, c_b, z_a, z_b = new(BF16, m, 9 * c), new(BF16, m, 9 * c), new(BF16, m, co), new(BF16, m, co)
    assert L.ocpg_conv3x3_mfma_fwd_splitk(_ptr(xm), _ptr(wm), _ptr(bias), n, h, wd, c, co, stride, sp, _ptr(part), _ptr(z_a), 1, _ptr(c_a), st) == 0
    assert L.ocpg_conv3x3_mfma_fwd_splitk_h16(_ptr(xm), _ptr(wm), _ptr(bias), n, h, wd, c, co, stride, sp, _ptr(part), _ptr(z_b), 1, _ptr(c_b), 1, st) == 0
    torch.cuda.synchronize()
    assert torch.equal(z_a, z_b) and torch.equal(c_a, c_b) and bool((z_a.float() != 7.0).any())
    for bad in (0, 3):
        y_p, outs = new(BF16, r, cout), [new(torch.float32, r, cin), new(BF16, cout, cin), new(BF16, cout)]
        z_p, c_p, part_p = new(BF16, m, co), new(BF16, m, 9 * c), new(torch.float32, sp, m, co)
        assert L.ocpg_small_linear_fwd_h16(_ptr(x), 1, _ptr(w), _ptr(b), r, cin, cout, 1, _ptr(y_p), bad, st) == -1010
        assert L.ocpg_small_linear_bwd_h16(_ptr(gy), 1, _ptr(x), 1, _ptr(w), _ptr(y_a), r, cin, cout, *[_ptr(t) for t in outs], bad, st) == -1010
        assert L.ocpg_conv3x3_mfma_fwd_splitk_h16(_ptr(xm), _ptr(wm), _ptr(bias), n, h, wd, c, co, stride, sp, _ptr(part_p), _ptr(z_p), 1, _ptr(c_p), bad,
                                                  st) == -1010
        torch.cuda.synchronize()
        for t in [y_p, z_p, c_p, part_p] + outs:
            assert bool((t.float() == 7.0).all())


# ---- 3. non-finite values and overflow ---------------------------------------------------------------------------------------------
def test_small_linear_fp16_nan_inf_and_overflow_as_the_library_path(dev):
    """An fp32 input of 1e6 (inf after the fp16 cast), a NaN, an inf, and a finite product past 65504 (40000 x 2: inf in fp16 as ATen's
    cast makes it): y has inf / NaN exactly where F.linear under fp16 autocast has them and equal finite values elsewhere (w = 2 I, so
    every finite y is 2 x, exact).  No clamping, no saturation."""
    from ocpg_amd.models import amp_cache
    g = torch.Generator(device=dev).manual_seed(3)
    x = torch.randn(4, 64, device=dev, generator=g)
    x[0, 0], x[1, 1], x[2, 2], x[3, 3] = 1e6, float("nan"), float("inf"), 40000.0
    w = (2.0 * torch.eye(64, device=dev)).to(H16)
    with torch.autocast("cuda", dtype=H16):
        assert amp_cache._small_linear_ok(x.requires_grad_(True), w, None)
        y = amp_cache.SmallLinearFunction.apply(x, w, None).detach().float()
        yr = torch.nn.functional.linear(x, w, None).detach().float()
    assert math.isinf(yr[0, 0].item()) and math.isnan(yr[1, 1].item()) and math.isinf(yr[2, 2].item()) and yr[3, 3].item() == math.inf
    assert y[3, 3].item() == math.inf and y[0, 0].item() == math.inf and y[2, 2].item() == math.inf and math.isnan(y[1, 1].item())
    assert torch.equal(torch.isnan(y), torch.isnan(yr))
    assert torch.equal(torch.isinf(y), torch.isinf(yr)) and torch.equal(y[torch.isinf(y)], yr[torch.isinf(yr)])        # same places, same signs
    fin = torch.isfinite(yr)
    assert bool(fin.any()) and torch.equal(y[fin], yr[fin])


# ---- 4. gates -------------------------------------------------------------------------------------------------------------------------
def test_small_linear_gates_refuse_mixed_16_bit_operands_and_honour_the_fp16_switch(dev, monkeypatch):
    from ocpg_amd.models import amp_cache
    x32 = torch.zeros(50, 256, device=dev)
    ops = {dt: (torch.zeros(50, 256, device=dev, dtype=dt), torch.zeros(256, 256, device=dev, dtype=dt), torch.zeros(256, device=dev, dtype=dt))
           for dt in (H16, BF16)}
    for ac in (H16, BF16):
        other = BF16 if ac == H16 else H16
        with torch.autocast("cuda", dtype=ac):
            x, w, b = ops[ac]
            xo, wo, bo = ops[other]
            assert amp_cache._small_linear_ok(x, w, b) and amp_cache._small_linear_ok(x32, w, b) and amp_cache._small_linear_ok(x, w, None)
            assert not amp_cache._small_linear_ok(xo, w, b)          # fp16 x with a bf16 w, and the reverse
            assert not amp_cache._small_linear_ok(x, wo, b)
            assert not amp_cache._small_linear_ok(x, w, bo)
            assert not amp_cache._small_linear_ok(xo, wo, bo)        # the other type throughout: not the autocast dtype
            assert not amp_cache._small_linear_ok(x32, wo, bo)
    monkeypatch.setattr(amp_cache, "SMALL_LINEAR_FP16", False)
    with torch.autocast("cuda", dtype=H16):
        assert not amp_cache._small_linear_ok(*ops[H16]) and not amp_cache._small_linear_ok(x32, *ops[H16][1:])
    with torch.autocast("cuda", dtype=BF16):
        assert amp_cache._small_linear_ok(*ops[BF16]) and amp_cache._small_linear_ok(x32, *ops[BF16][1:])


def test_splitk_conv_gate_follows_the_autocast_dtype(dev, monkeypatch):
    """amp_cache.Conv2d: the split-K branch serves a map and a weight that are both of the autocast dtype; a bf16 map with an fp16 weight
    (or the reverse) is never launched and takes _conv_forward; OCPG_SPLITK_3X3_FP16=0 returns the fp16 call to the library, not the bf16 one."""
    from ocpg_amd import _lib
    from ocpg_amd.models import amp_cache
    conv = amp_cache.Conv2d(256, 64, 3, stride=2, padding=1).to(dev).to(memory_format=CL)
    x = torch.randn(1, 256, 5, 5, device=dev).contiguous(memory_format=CL)

    def run(ac, xdt, wdt):
        conv.to(wdt)
        calls = _lib.census(True)
        try:
            with torch.autocast("cuda", dtype=ac), torch.no_grad():
                y = conv(x.to(xdt))
            torch.cuda.synchronize()
        finally:
            counts = dict(calls)
            _lib.census(False)
        assert y.dtype == ac
        return {k for k in counts if k.startswith("ocpg_conv3x3_mfma_") and "splits" not in k}
    assert run(H16, H16, H16) == {"ocpg_conv3x3_mfma_fwd_splitk_h16"}
    assert run(BF16, BF16, BF16) == {"ocpg_conv3x3_mfma_fwd_splitk"}
    for ac, xdt, wdt in ((H16, H16, BF16), (H16, BF16, H16), (BF16, H16, BF16), (BF16, BF16, H16), (H16, BF16, BF16), (BF16, H16, H16)):
        assert run(ac, xdt, wdt) == set(), (ac, xdt, wdt)
    monkeypatch.setattr(amp_cache, "SPLITK_3X3_FP16", False)
    assert run(H16, H16, H16) == set()
    assert run(BF16, BF16, BF16) == {"ocpg_conv3x3_mfma_fwd_splitk"}


# ---- 5. the neck's split-K convolution ---------------------------------------------------------------------------------------------------
def _splitk_case(dev, n, c, co, h, w, stride, dtype):
    from ocpg_amd import _lib
    from ocpg_amd.models.ops.functions import conv_bn_func as f
    assert int(_lib.lib().ocpg_conv3x3_mfma_splits(n, h, w, c, co, stride)) > 1
    g = torch.Generator(device="cpu").manual_seed(n * 100 + c + h)
    x = torch.randn(n, c, h, w, generator=g).to(dev).to(dtype).contiguous(memory_format=CL)
    wt = (torch.randn(co, c, 3, 3, generator=g) * (2.0 / (9 * c)) ** 0.5).to(dev).to(dtype).contiguous(memory_format=CL)
    b = (torch.randn(co, generator=g) * 0.1).to(dev).to(dtype)
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    go = torch.randn(n, co, ho, wo, generator=g).to(dev).to(dtype).contiguous(memory_format=CL)
    xi, wi, bi = x.clone().requires_grad_(True), wt.clone().requires_grad_(True), b.clone().requires_grad_(True)
    calls = _lib.census(True)
    try:
        y = f.conv3x3_splitk(xi, wi, bi, stride)
        assert y.shape == (n, co, ho, wo) and y.is_contiguous(memory_format=CL) and y.dtype == dtype
        gx, gw, gb = torch.autograd.grad(y, (xi, wi, bi), go)
        torch.cuda.synchronize()
    finally:
        counts = dict(calls)
        _lib.census(False)
    assert gx.dtype == dtype and gw.dtype == dtype and gb.dtype == dtype
    xr, wr, br = x.float().requires_grad_(True), wt.float().requires_grad_(True), b.float().requires_grad_(True)
    yr = torch.nn.functional.conv2d(xr, wr, br, stride, 1)
    gxr, gwr, gbr = torch.autograd.grad(yr, (xr, wr, br), go.float())
    return counts, (_rel(y, yr), _rel(gx, gxr), _rel(gw, gwr), _rel(gb, gbr))


@pytest.mark.parametrize("n,c,co,h,w,stride", [(1, 256, 64, 5, 5, 2), (2, 512, 128, 7, 9, 1), (10, 2048, 256, 12, 20, 2)])
def test_conv3x3_splitk_fp16_kernel(dev, n, c, co, h, w, stride):
    """The protocol and shapes of test_model_gpu.py::test_conv3x3_splitk_kernel in fp16 against F.conv2d in fp32 on the fp16-rounded
    operands; the census shows the two _h16 symbols once each and no un-suffixed conv3x3 symbol; the same call in bf16 shows the symbols it
    always used and no _h16 one."""
    counts, (ry, rgx, rgw, rgb) = _splitk_case(dev, n, c, co, h, w, stride, H16)
    print(f"conv3x3 split-K fp16 n{n} c{c} co{co} {h}x{w} s{stride}: rel(y) {ry:.3e} rel(gx) {rgx:.3e} rel(gw) {rgw:.3e} rel(gb) {rgb:.3e}; {counts}")
    assert counts.get("ocpg_conv3x3_mfma_fwd_splitk_h16") == 1 and counts.get("ocpg_conv3x3_mfma_dgrad_w_h16") == 1, counts
    assert not [k for k in counts if k.startswith("ocpg_conv3x3_mfma_") and not k.endswith("_h16") and not k.endswith("_splits")], counts
    assert ry <= 7.5e-4, ry
    assert rgx <= 1.9e-3 and rgw <= 1.9e-3 and rgb <= 1.9e-3, (rgx, rgw, rgb)
    counts, rels = _splitk_case(dev, n, c, co, h, w, stride, BF16)
    assert counts.get("ocpg_conv3x3_mfma_fwd_splitk") == 1 and counts.get("ocpg_conv3x3_mfma_dgrad") == 1, counts
    assert not [k for k in counts if k.endswith("_h16")], counts
    assert rels[0] <= 6e-3 and max(rels[1:]) <= 1.5e-2, rels          # the bf16 test's own bounds


def test_conv3x3_splitk_refuses_mixed_16_bit_operands(dev):
    from ocpg_amd.models.ops.functions import conv_bn_func as f
    x = torch.randn(1, 256, 5, 5, device=dev).to(H16).contiguous(memory_format=CL)
    wt = torch.randn(64, 256, 3, 3, device=dev).to(BF16).contiguous(memory_format=CL)
    with pytest.raises(RuntimeError, match="16-bit dtype"):
        f.conv3x3_splitk(x, wt, None, 2)
    with pytest.raises(RuntimeError, match="16-bit dtype"):
        f.conv3x3_splitk(x.to(BF16), wt.to(H16), None, 2)


# ---- 6. the tiny model --------------------------------------------------------------------------------------------------------------------
NEW = ("ocpg_small_linear_fwd_h16", "ocpg_small_linear_bwd_h16", "ocpg_conv3x3_mfma_fwd_splitk_h16")


def test_tiny_step_under_fp16_runs_the_few_row_linears_on_the_fp16_kernels(dev, monkeypatch):
    """e2e_tiny, one bench.forward_backward per leg on ONE model (no optimizer step in between; gradients cleared): fp32, bf16, fp16 with
    GradScaler(init_scale=64.0), and fp16 with both new switches off.  fp16 census: ocpg_small_linear_fwd_h16 > 0, as many _bwd_h16, no
    un-suffixed small_linear symbol; bf16 census: the un-suffixed symbols only; switches off: none of the three new symbols.  Both fp16
    losses are finite and within 2e-2 relative of the fp32 loss, and every parameter with a gradient in the bf16 run has a finite one."""
    _paths()
    import bench
    from ocpg_amd import _lib
    from ocpg_amd.models import amp_cache
    from ocpg_amd.util.misc import NestedTensor
    meta, args, model, crit = _tiny(dev)
    x, mask, targets, text = _tiny_batch(meta, dev)

    def leg(amp, scaler=None):
        model.zero_grad(set_to_none=True)
        crit.iter = 0
        calls = _lib.census(True)
        try:
            loss = bench.forward_backward(model, crit, NestedTensor(x.clone(), mask.clone()), text, targets, amp, scaler=scaler)
            torch.cuda.synchronize()
        finally:
            counts = dict(calls)
            _lib.census(False)
        return float(loss), counts, {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
    loss32, _, _ = leg(None)
    _, c_bf, g_bf = leg(BF16)
    loss16, c_16, g_16 = leg(H16, torch.amp.GradScaler("cuda", init_scale=64.0))
    monkeypatch.setattr(amp_cache, "SMALL_LINEAR_FP16", False)
    monkeypatch.setattr(amp_cache, "SPLITK_3X3_FP16", False)
    loss_off, c_off, _ = leg(H16, torch.amp.GradScaler("cuda", init_scale=64.0))
    pick = lambda c: {k: v for k, v in c.items() if "small_linear" in k or "splitk" in k}      # noqa: E731
    print(f"tiny step: fp32 loss {loss32:.6f}, fp16 {loss16:.6f} (relative {abs(loss16 - loss32) / abs(loss32):.3e}), fp16 switches off {loss_off:.6f} "
          f"(relative {abs(loss_off - loss32) / abs(loss32):.3e}); census fp16 {pick(c_16)}, bf16 {pick(c_bf)}, off {pick(c_off)}")
    assert c_16.get("ocpg_small_linear_fwd_h16", 0) > 0, c_16
    assert c_16.get("ocpg_small_linear_bwd_h16", 0) == c_16["ocpg_small_linear_fwd_h16"], c_16
    assert not c_16.get("ocpg_small_linear_fwd", 0) and not c_16.get("ocpg_small_linear_bwd", 0), c_16
    assert c_bf.get("ocpg_small_linear_fwd", 0) > 0 and c_bf.get("ocpg_small_linear_bwd", 0) > 0, c_bf
    assert not [k for k in NEW if c_bf.get(k, 0)], c_bf
    assert not [k for k in NEW if c_off.get(k, 0)], c_off
    assert not c_off.get("ocpg_small_linear_fwd", 0) and not c_off.get("ocpg_small_linear_bwd", 0), c_off
    for loss in (loss16, loss_off):
        assert math.isfinite(loss) and abs(loss - loss32) <= 2e-2 * abs(loss32), (loss, loss32)
    assert g_bf and set(g_bf) <= set(g_16), sorted(set(g_bf) - set(g_16))
    bad = [k for k in g_bf if not torch.isfinite(g_16[k]).all()]
    assert not bad, bad
