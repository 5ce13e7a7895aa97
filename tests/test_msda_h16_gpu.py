"""16-bit-storage MSDeformAttn on the GPU (ocpg_msda_fwd_h16 / ocpg_msda_bwd_h16, MSDeformAttn(value_dtype=...), args.msda_value_dtype).

The reference's op is fp32 only, so the yardstick is the C oracle evaluated on the 16-bit inputs WIDENED to fp32 (exact): the kernels
compute in fp32 and round `out` once, so
    |out - ref| <= (u + 1e-4) |ref| + 1e-5,      u = 2^-8 (bfloat16) / 2^-11 (float16), no element exempt
(one round-to-nearest-even of an fp32 result + the fp32 summation-order term test_msda_gpu.py grants the fp32 kernels), and the fp32
gradients of the C entry point keep the fp32 tolerances of test_msda_gpu.py unchanged.

The fused front end has no 16-bit form yet (the module takes the un-fused op in 16-bit mode), so there is no fused-vs-unfused test here.
"""
import ctypes
import math
import os

import pytest
import torch

from cases import level_start

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
IDS = ["bf16", "fp16"]
U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
CODE = {torch.bfloat16: 1, torch.float16: 2}
CFG2 = [(48, 80), (24, 40), (12, 20), (6, 10)]
SELF_SHAPES = {"cfg2": CFG2, "cfg5": [(60, 108), (30, 54), (15, 27), (8, 14)], "cfg1_3lvl": [(32, 32), (16, 16), (8, 8)],
               "ragged": [(13, 7), (5, 9)]}


class _env:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _local_inputs(N, shapes_l, dtype, M=8, D=32, P=4, noise=1.5, outliers=0.02, seed=5):
    """Encoder-like sampling pattern (the module's initial ring: the head's direction, 1..P pixels from the query's own pixel) plus
    gaussian noise, a few far outliers and samples outside the map; value / grad_out are randn rounded to the 16-bit dtype (|out| << 65504)."""
    shapes, ls = level_start(shapes_l)
    S = int(shapes.prod(1).sum())
    L = len(shapes_l)
    g = torch.Generator().manual_seed(seed)
    refs = []
    for (h, w) in shapes_l:
        ys, xs = torch.meshgrid(torch.linspace(0.5, h - 0.5, h) / h, torch.linspace(0.5, w - 0.5, w) / w, indexing="ij")
        refs.append(torch.stack([xs.reshape(-1), ys.reshape(-1)], -1))
    ref = torch.cat(refs, 0)[None, :, None, None, None, :]
    th = torch.arange(M) * (2 * math.pi / M)
    grid = torch.stack([th.cos(), th.sin()], -1)
    grid = grid / grid.abs().max(-1, keepdim=True)[0]
    off = grid.view(1, 1, M, 1, 1, 2) * torch.arange(1, P + 1).view(1, 1, 1, 1, P, 1)
    off = off.expand(N, S, M, L, P, 2) + noise * torch.randn(N, S, M, L, P, 2, generator=g)
    norm = torch.tensor([[w, h] for h, w in shapes_l], dtype=torch.float32).view(1, 1, 1, L, 1, 2)
    loc = ref + off / norm
    far = torch.rand(N, S, M, L, P, 1, generator=g) < outliers
    loc = torch.where(far, torch.rand(N, S, M, L, P, 2, generator=g) * 1.3 - 0.15, loc).contiguous()
    value = torch.randn(N, S, M, D, generator=g).to(dtype)
    attn = torch.softmax(torch.randn(N, S, M, L * P, generator=g), -1).view(N, S, M, L, P)
    go = torch.randn(N, S, M * D, generator=g).to(dtype)
    return value, shapes, ls, loc, attn, go


def _random_inputs(N, shapes_l, Lq, M, D, P, dtype, seed=11):
    """Cross-attention-like inputs (as _full_size_inputs of test_msda_gpu.py): uniform locations in [-0.05, 1.05], softmax weights."""
    shapes, ls = level_start(shapes_l)
    S = int(shapes.prod(1).sum())
    L = len(shapes_l)
    g = torch.Generator().manual_seed(seed)
    value = torch.randn(N, S, M, D, generator=g).to(dtype)
    loc = torch.rand(N, Lq, M, L, P, 2, generator=g) * 1.1 - 0.05
    attn = torch.softmax(torch.randn(N, Lq, M, L * P, generator=g), -1).view(N, Lq, M, L, P)
    go = torch.randn(N, Lq, M * D, generator=g).to(dtype)
    return value, shapes, ls, loc, attn, go


def _c_backward(value, ds, dls, loc, attn, go, sel_state=None):
    """ocpg_msda_bwd_h16 itself: fp32 grad_value (the autograd wrapper rounds it to value's dtype), grad_loc, grad_attn."""
    from ocpg_amd._lib import check, lib, stream_ptr
    N, S, M, D = value.shape
    _, Lq, _, L, P, _ = loc.shape
    gv = torch.zeros(value.shape, dtype=torch.float32, device=value.device)
    gl, ga = torch.empty_like(loc), torch.empty_like(attn)
    hs = getattr(ds, "_ocpg_host", None)
    check(lib().ocpg_msda_bwd_h16(value.data_ptr(), ds.data_ptr(), dls.data_ptr(), loc.data_ptr(), attn.data_ptr(), go.data_ptr(),
                                  N, S, M, D, L, Lq, P, gv.data_ptr(), gl.data_ptr(), ga.data_ptr(),
                                  ctypes.c_void_p(hs.data_ptr()) if hs is not None else None,
                                  sel_state.data_ptr() if sel_state is not None else None, CODE[value.dtype], stream_ptr()),
          "ocpg_msda_bwd_h16")
    return gv, gl, ga


def _assert_forward(out, ref, dtype, what):
    assert out.dtype == dtype
    err = (out.float().cpu() - ref).abs()
    bound = (U[dtype] + 1e-4) * ref.abs() + 1e-5
    ratio = (err / bound).max().item()
    print(f"forward {what}: worst element at {ratio:.3f} of the bound, max|ref| {ref.abs().max().item():.3f}")
    assert ratio <= 1.0, (what, ratio)


def _assert_backward(gv32, gv16, gl, ga, ogv, ogl, oga, dtype, what):
    assert gv32.dtype == torch.float32 and gl.dtype == torch.float32 and ga.dtype == torch.float32 and gv16.dtype == dtype
    assert torch.allclose(gv32.cpu(), ogv, rtol=1e-3, atol=1e-4), what
    assert (gl.cpu() - ogl).abs().max() <= 2e-5 * ogl.abs().max(), what
    assert torch.allclose(ga.cpu(), oga, rtol=1e-3, atol=1e-4), what
    # the autograd-level grad_value is that fp32 result rounded once: the forward's bound on top of the fp32 tolerance
    err16 = (gv16.float().cpu() - ogv).abs()
    assert (err16 <= (U[dtype] + 1e-4 + 1e-3) * ogv.abs() + 1e-4 + 1e-5).all(), (what, (err16 / (ogv.abs() + 1e-4)).max().item())


def _run_case(dev, value, shapes, ls, loc, attn, go, dtype, envs, host_shapes, what):
    from oracle import msda as om
    from ocpg_amd.models.ops.functions import ms_deform_attn_backward, ms_deform_attn_forward
    oc = om.msda_c_forward(value.float(), shapes, ls, loc, attn)
    ogv, ogl, oga = om.msda_c_backward(value.float(), shapes, ls, loc, attn, go.float())
    dv, dl, da, dg = (t.to(dev) for t in (value, loc, attn, go))
    ds, dls = shapes.to(dev), ls.to(dev)
    if host_shapes:
        ds._ocpg_host = shapes
    for env in envs:
        with _env(**env):
            out = ms_deform_attn_forward(dv, ds, dls, dl, da)
            gv16, gl2, ga2 = ms_deform_attn_backward(dv, ds, dls, dl, da, dg)
            gv32, gl, ga = _c_backward(dv, ds, dls, dl, da, dg)
        _assert_forward(out, oc, dtype, f"{what} {env}")
        _assert_backward(gv32, gv16, gl, ga, ogv, ogl, oga, dtype, f"{what} {env}")
        assert torch.equal(gl, gl2) and torch.equal(ga, ga2), (what, env)       # same kernels, no atomics on this side


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", list(SELF_SHAPES))
def test_self_attention_shapes_vs_c_oracle(dev, dtype, name):
    """Forward and backward at the four self-attention shapes of test_msda_gpu.py, one frame, under the default route (column scatter +
    row gather), the output-tiled grad_value kernels, the row kernel with atomic scatter (OCPG_MSDA_COL=0) and the generic backward the
    forced single-level column scatter, which reads fp32 only, falls to (OCPG_MSDA_COL_LP=1)."""
    value, shapes, ls, loc, attn, go = _local_inputs(1, SELF_SHAPES[name], dtype)
    _run_case(dev, value, shapes, ls, loc, attn, go, dtype, ({}, {"OCPG_MSDA_TILE": "1"}, {"OCPG_MSDA_COL": "0"}, {"OCPG_MSDA_COL_LP": "1"}),
              True, name)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("lanes", ["4", "8"])
def test_both_lane_mappings_vs_c_oracle(dev, dtype, lanes):
    """OCPG_MSDA_H16_LANES forces 4 or 8 channels per lane in the forward and the gather: both are held to the same bounds."""
    value, shapes, ls, loc, attn, go = _local_inputs(1, CFG2, dtype, seed=6)
    _run_case(dev, value, shapes, ls, loc, attn, go, dtype, ({"OCPG_MSDA_H16_LANES": lanes},), True, f"lanes={lanes}")
    value, shapes, ls, loc, attn, go = _local_inputs(1, [(16, 24), (8, 12)], dtype, M=4, D=16, seed=7)
    _run_case(dev, value, shapes, ls, loc, attn, go, dtype, ({"OCPG_MSDA_H16_LANES": lanes},), True, f"D=16 lanes={lanes}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_cross_attention_generic_and_empty_shapes(dev, dtype):
    from ocpg_amd.models.ops.functions import ms_deform_attn_backward, ms_deform_attn_forward
    # cross-attention (Lq = 25 != S): row kernel with the fp32 atomic scatter
    _run_case(dev, *_random_inputs(2, CFG2, 25, 8, 32, 4, dtype), dtype, ({},), True, "Lq=25")
    # head dimensions without a fast path: generic kernels (D = 30: not a multiple of 4; D = 71: odd)
    _run_case(dev, *_random_inputs(2, [(9, 11), (4, 6)], 37, 2, 30, 3, dtype, seed=12), dtype, ({},), False, "D=30")
    _run_case(dev, *_random_inputs(1, [(9, 11), (4, 6)], 123, 3, 71, 2, dtype, seed=13), dtype, ({},), True, "D=71 self-sized")
    # a value view that misses the 16-byte alignment of the fast kernels takes the generic ones: same results
    value, shapes, ls, loc, attn, go = _random_inputs(1, [(9, 11), (4, 6)], 40, 2, 32, 4, dtype, seed=14)
    flat = torch.empty(value.numel() + 1, dtype=dtype, device=dev)
    shifted = flat[1:].view(value.shape)
    shifted.copy_(value)
    assert shifted.data_ptr() % 16 != 0 and shifted.is_contiguous()
    ds, dls = shapes.to(dev), ls.to(dev)
    a = ms_deform_attn_forward(value.to(dev), ds, dls, loc.to(dev), attn.to(dev))
    b = ms_deform_attn_forward(shifted, ds, dls, loc.to(dev), attn.to(dev))
    assert ((a.float() - b.float()).abs() <= 2 * U[dtype] * a.float().abs() + 1e-5).all()
    # Lq = 0
    shapes, ls = level_start([(3, 4)])
    value = torch.randn(3, 12, 2, 8, device=dev).to(dtype)
    loc = torch.rand(3, 0, 2, 1, 2, 2, device=dev)
    attn = torch.rand(3, 0, 2, 1, 2, device=dev)
    out = ms_deform_attn_forward(value, shapes.to(dev), ls.to(dev), loc, attn)
    assert out.shape == (3, 0, 16) and out.dtype == dtype
    gv, gl, ga = ms_deform_attn_backward(value, shapes.to(dev), ls.to(dev), loc, attn, out)
    assert gv.dtype == dtype and gv.shape == value.shape and not gv.any() and gl.shape == loc.shape and ga.shape == attn.shape


def _shifted(t, nbytes):
    """a contiguous copy of t whose data pointer sits `nbytes` past a 16-byte boundary"""
    k = nbytes // t.element_size()
    flat = torch.empty(t.numel() + k, dtype=t.dtype, device=t.device)
    out = flat[k:].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 == nbytes and out.is_contiguous()
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("which", ["grad_out", "value", "loc", "grad_value"])
def test_backward_with_a_buffer_off_the_16_byte_boundary(dev, dtype, which):
    """Alignment is settled before anything is launched: the whole backward still returns the oracle's gradients (generic kernels, or the
    row kernel when only loc / grad_value miss what the tiled kernels want), and the two halves answer -2000 without touching their outputs."""
    from oracle import msda as om
    from ocpg_amd._lib import lib, stream_ptr
    value, shapes, ls, loc, attn, go = _local_inputs(1, [(16, 24), (8, 12)], dtype, seed=8)
    ogv, ogl, oga = om.msda_c_backward(value.float(), shapes, ls, loc, attn, go.float())
    dv, dl, da, dg = (t.to(dev) for t in (value, loc, attn, go))
    ds, dls = shapes.to(dev), ls.to(dev)
    ds._ocpg_host = shapes
    N, S, M, D = value.shape
    L, P = loc.shape[3], loc.shape[4]
    gv = torch.zeros(value.shape, dtype=torch.float32, device=dev)
    if which == "grad_out":
        dg = _shifted(dg, 2)
    elif which == "value":
        dv = _shifted(dv, 8)
    elif which == "loc":
        dl = _shifted(dl, 8)
    else:
        gv = _shifted(gv, 4)
    gl, ga = torch.empty_like(dl), torch.empty_like(da)
    hs = ctypes.c_void_p(shapes.data_ptr())
    state = torch.zeros(8, dtype=torch.int32, device=dev)
    rc = lib().ocpg_msda_bwd_h16(dv.data_ptr(), ds.data_ptr(), dls.data_ptr(), dl.data_ptr(), da.data_ptr(), dg.data_ptr(), N, S, M, D, L, S, P,
                                 gv.data_ptr(), gl.data_ptr(), ga.data_ptr(), hs, state.data_ptr(), CODE[dtype], stream_ptr())
    assert rc == 0, rc
    assert torch.allclose(gv.cpu(), ogv, rtol=1e-3, atol=1e-4)
    assert (gl.cpu() - ogl).abs().max() <= 2e-5 * ogl.abs().max() and torch.allclose(ga.cpu(), oga, rtol=1e-3, atol=1e-4)
    assert not state.any()                      # the path-selection kernels did not run
    # the halves: the one that reads the shifted buffer refuses with -2000 and writes nothing
    if which != "value":
        gv2 = torch.zeros(value.shape, dtype=torch.float32, device=dev)
        if which == "grad_value":
            gv2 = _shifted(gv2, 4)
        rc = lib().ocpg_msda_bwd_value_h16(dl.data_ptr(), da.data_ptr(), dg.data_ptr(), N, S, M, D, L, S, P, gv2.data_ptr(), hs, state.data_ptr(),
                                           CODE[dtype], stream_ptr())
        torch.cuda.synchronize()
        assert rc == -2000 and not gv2.any() and not state.any()
    if which in ("grad_out", "value"):
        gl2, ga2 = torch.full_like(dl, 7.0), torch.full_like(da, 7.0)
        rc = lib().ocpg_msda_bwd_locattn_h16(dv.data_ptr(), ds.data_ptr(), dls.data_ptr(), dl.data_ptr(), da.data_ptr(), dg.data_ptr(), N, S, M, D,
                                             L, S, P, gl2.data_ptr(), ga2.data_ptr(), CODE[dtype], stream_ptr())
        torch.cuda.synchronize()
        assert rc == -2000 and (gl2 == 7.0).all() and (ga2 == 7.0).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_argument_contract(dev, dtype):
    from ocpg_amd._lib import lib, stream_ptr
    from ocpg_amd.models.ops.functions import MSDeformAttnFunction, ms_deform_attn_forward
    value, shapes, ls, loc, attn, go = _random_inputs(1, [(9, 11), (4, 6)], 5, 2, 32, 4, dtype)
    dv, ds, dls, dl, da = value.to(dev), shapes.to(dev), ls.to(dev), loc.to(dev), attn.to(dev)
    with pytest.raises(RuntimeError, match="sampling_loc must be float32"):
        ms_deform_attn_forward(dv, ds, dls, dl.to(dtype), da)
    with pytest.raises(RuntimeError, match="attn_weight must be float32"):
        ms_deform_attn_forward(dv, ds, dls, dl, da.to(dtype))
    with pytest.raises(RuntimeError, match="contiguous"):
        ms_deform_attn_forward(torch.randn(1, 123, 2, 64, device=dev).to(dtype)[..., ::2], ds, dls, dl, da)
    # an unknown dtype code: invalid-argument status, nothing written
    out = torch.full((1, 5, 64), 7.0, device=dev).to(dtype)
    rc = lib().ocpg_msda_fwd_h16(dv.data_ptr(), ds.data_ptr(), dls.data_ptr(), dl.data_ptr(), da.data_ptr(), 1, 123, 2, 32, 2, 5, 4,
                                 out.data_ptr(), None, 0, stream_ptr())
    torch.cuda.synchronize()
    assert rc == -1015 and (out.float() == 7.0).all()
    gv = torch.zeros(value.shape, device=dev)
    gl, ga = torch.full_like(dl, 7.0), torch.full_like(da, 7.0)
    rc = lib().ocpg_msda_bwd_h16(dv.data_ptr(), ds.data_ptr(), dls.data_ptr(), dl.data_ptr(), da.data_ptr(), go.to(dev).data_ptr(), 1, 123, 2, 32,
                                 2, 5, 4, gv.data_ptr(), gl.data_ptr(), ga.data_ptr(), None, None, 3, stream_ptr())
    torch.cuda.synchronize()
    assert rc == -1019 and not gv.any() and (gl == 7.0).all() and (ga == 7.0).all()
    # autograd: out and the gradient of value in value's dtype, grad_loc / grad_attn fp32
    v, l, a = dv.clone().requires_grad_(True), dl.clone().requires_grad_(True), da.clone().requires_grad_(True)
    o = MSDeformAttnFunction.apply(v, ds, dls, l, a, 64)
    assert o.dtype == dtype
    o.float().square().sum().backward()
    assert v.grad.dtype == dtype and l.grad.dtype == torch.float32 and a.grad.dtype == torch.float32


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_grad_value_path_selection_with_16_bit_grad_out(dev, dtype):
    """The scenario of test_grad_value_path_selection_follows_the_offsets with 16-bit value / grad_out: the call site's state moves to the
    output-tiled kernels on spread-out offsets and back, and every call returns the fixed path's grad_value."""
    near = [t.to(dev) if i != 1 else t for i, t in enumerate(_local_inputs(2, CFG2, dtype, noise=0.3, outliers=0.0, seed=3))]
    wide = [t.to(dev) if i != 1 else t for i, t in enumerate(_local_inputs(2, CFG2, dtype, noise=4.0, outliers=0.08, seed=4))]
    shapes = near[1]
    ds, dls = shapes.to(dev), near[2]
    ds._ocpg_host = shapes
    state = torch.zeros(8, dtype=torch.int32, device=dev)
    want = {}
    for name, (value, _, _, loc, attn, go) in (("near", near), ("wide", wide)):
        want[name] = _c_backward(value, ds, dls, loc, attn, go)[0]
    seen = []
    for name in ("near", "wide", "wide", "wide", "near", "near", "near"):
        value, _, _, loc, attn, go = near if name == "near" else wide
        ran = int(state[3])                                  # the path THIS call takes
        gv = _c_backward(value, ds, dls, loc, attn, go, sel_state=state)[0]
        st = state.tolist()
        seen.append((name, ran, st[3], st[6], st[7]))
        assert (gv - want[name]).abs().max() <= 2e-5 * want[name].abs().max(), seen
        assert st[0] == 0 and st[1] == 0 and st[2] == 0 and st[5] == 0, st
        assert st[7] > 0 and 0 <= st[6] <= st[7], st
    paths = [r for _, r, _, _, _ in seen]
    assert paths == [0, 0, 1, 1, 1, 0, 0], seen
    assert seen[1][3] * 100 > 6 * seen[1][4] and seen[0][3] * 100 < 6 * seen[0][4], seen


def _ulp_at(x, dtype):
    return 2.0 ** (math.floor(math.log2(x)) - (7 if dtype == torch.bfloat16 else 10))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("pad", [False, True], ids=["nopad", "pad"])
def test_module_in_16_bit_mode_vs_emulation(dev, dtype, pad):
    """MSDeformAttn(value_dtype=dtype) at the config-#2 encoder shape against torch ops with the same cast points: F.linear in the 16-bit
    dtype -> padding fill -> fp32 sampling of the widened value at the module's own (fp32) locations / weights -> one rounding -> F.linear.
    Two library GEMMs make the tolerance underivable; it comes from the referee: twice the distance between that emulation and the same
    emulation accumulated in fp64, floored at one ulp of the dtype at max|out| (as test_model_gpu.py does for the full model)."""
    import torch.nn.functional as F
    from oracle.msda import msda_torch
    from ocpg_amd import _lib
    from ocpg_amd.models.ops.modules import MSDeformAttn
    shapes, ls = level_start(CFG2)
    S = int(shapes.prod(1).sum())
    g = torch.Generator().manual_seed(11)
    m = MSDeformAttn(256, 4, 8, 4, value_dtype=dtype)
    with torch.no_grad():
        m.sampling_offsets.weight.copy_(torch.randn(m.sampling_offsets.weight.shape, generator=g) * 0.05)
        m.attention_weights.weight.copy_(torch.randn(m.attention_weights.weight.shape, generator=g) * 0.2)
        m.attention_weights.bias.copy_(torch.randn(m.attention_weights.bias.shape, generator=g) * 0.5)
    m.to(dev)
    N = 2
    refs = []
    for (h, w) in CFG2:
        ys, xs = torch.meshgrid((torch.arange(h) + 0.5) / h, (torch.arange(w) + 0.5) / w, indexing="ij")
        refs.append(torch.stack([xs.reshape(-1), ys.reshape(-1)], -1))
    ref = torch.cat(refs, 0)[None, :, None, :].expand(N, S, 4, 2).contiguous().to(dev)
    q = torch.randn(N, S, 256, generator=g).to(dev).requires_grad_(True)
    src = torch.randn(N, S, 256, generator=g).to(dev).requires_grad_(True)
    go = torch.randn(N, S, 256, generator=g).to(dev)
    mask = None
    if pad:
        mask = torch.zeros(N, S, dtype=torch.bool)
        mask[1, 3000:3600] = True
        mask = mask.to(dev)
    ds, dls = shapes.to(dev), ls.to(dev)
    ds._ocpg_host = shapes
    calls = _lib.census(True)
    try:
        out, loc, attn = m(q, ref, src, ds, dls, mask)
        grads = torch.autograd.grad((out.float() * go).sum(), [q, src] + list(m.parameters()))
    finally:
        _lib.census(False)
    assert out.dtype == dtype and loc.dtype == torch.float32 and attn.dtype == torch.float32
    assert calls.get("ocpg_msda_fwd_h16") == 1 and calls.get("ocpg_msda_bwd_h16") == 1, calls
    assert not [k for k in calls if k.startswith("ocpg_msda_") and not k.endswith("_h16")], calls
    assert all(torch.isfinite(g_).all() for g_ in grads) and grads[1].abs().max() > 0 and grads[0].abs().max() > 0
    assert int(m._sel_state[7]) > 0             # the call site's path-selection state was used by the 16-bit backward

    def emulate(acc):
        with torch.no_grad():
            x, wv, bv = src.detach().to(dtype), m.value_proj.weight.to(dtype), m.value_proj.bias.to(dtype)
            wo, bo = m.output_proj.weight.to(dtype), m.output_proj.bias.to(dtype)
            if acc == torch.float64:
                value = (x.double() @ wv.double().t() + bv.double()).to(dtype)
            else:
                value = F.linear(x, wv, bv)
            if mask is not None:
                value = value.masked_fill(mask[..., None], 0.0)
            sampled = msda_torch(value.view(N, S, 8, 32).to(acc), shapes.tolist(), loc.detach().to(acc), attn.detach().to(acc)).to(dtype)
            if acc == torch.float64:
                return sampled.double() @ wo.double().t() + bo.double()
            return F.linear(sampled, wo, bo).double()

    e32, e64 = emulate(torch.float32), emulate(torch.float64)
    d_ref = (e32 - e64).abs().max().item()
    d_mod = (out.detach().double() - e32).abs().max().item()
    mx = e64.abs().max().item()
    tol = max(2.0 * d_ref, _ulp_at(mx, dtype))
    print(f"module ({dtype}, pad={pad}): max|module - emulation| {d_mod:.3e}; referee: max|emulation - fp64 emulation| {d_ref:.3e}; "
          f"max|out| {mx:.3f}, one ulp there {_ulp_at(mx, dtype):.3e}, tolerance {tol:.3e}")
    assert d_mod <= tol, (d_mod, d_ref, tol)


def _tiny(dev, fixture="e2e_tiny", **over):
    """The tiny end-to-end model of a committed fixture (e2e_tiny: ResNet; e2e_swin: the tiny Video-Swin of test_graph_gpu.py -- the
    backbone the project runs under fp16, config #5; the frozen-BN kernels of the ResNet body have no fp16 form)."""
    import cases
    import model_checks
    from conftest import Golden
    meta = Golden(fixture).meta
    if "swin_cfg" in meta:
        import synth
        from ocpg_amd.models import build_model
        args = cases.default_args(device=str(dev), video_swin_cfg=meta["swin_cfg"], **meta["cfg"], **over)
        model, crit, _ = build_model(args)
        missing = model.load_state_dict(synth.synth_state_dict(meta["float_shapes"], seed=meta["seed"]), strict=False)
        assert not missing.unexpected_keys and all("relative_position_index" in k for k in missing.missing_keys)
        for m in model.modules():
            if isinstance(m, torch.nn.Dropout):
                m.p = 0.0
        model.to(dev), crit.to(dev)
    else:
        args, model, crit = model_checks.build_product(meta, dev, **over)
    model_checks.to_channels_last(model)
    model.train(), crit.train()
    return meta, args, model, crit


def _tiny_batch(meta, dev):
    import cases
    import model_checks
    B, T, H, W = meta.get("B", 2), meta["T"], meta["H"], meta["W"]
    x, mask, targets = cases.e2e_inputs(B, T, H, W, meta["pad_sizes" if "swin_cfg" in meta else "nopad_sizes"], dev)
    return x, mask, targets, model_checks.text_for(B, dev)


@pytest.mark.parametrize("dtype,word", [(torch.bfloat16, "bf16"), (torch.float16, "fp16"), (torch.bfloat16, "autocast")],
                         ids=["bf16", "fp16", "autocast-bf16"])
def test_tiny_training_step_in_16_bit_mode(dev, dtype, word):
    """e2e_tiny-sized model (bf16: the ResNet fixture; fp16 + GradScaler: the tiny Video-Swin fixture) under autocast with the 16-bit value path: finite losses, a finite gradient for every parameter that has one in the
    default mode, one optimizer step changes the weights; the census shows the 16-bit op and no fp32 MSDeformAttn forward."""
    import bench
    from ocpg_amd import _lib
    from ocpg_amd.util.misc import NestedTensor
    fixture = "e2e_swin" if dtype == torch.float16 else "e2e_tiny"
    meta, args, model, crit = _tiny(dev, fixture, msda_value_dtype=word)
    _, _, base, base_crit = _tiny(dev, fixture)
    x, mask, targets, text = _tiny_batch(meta, dev)
    scaler = torch.amp.GradScaler("cuda", init_scale=64.0) if dtype == torch.float16 else None      # (65536 overflows the tiny model's fp16 backward)
    base_crit.iter = 0
    bench.forward_backward(base, base_crit, NestedTensor(x.clone(), mask.clone()), text, targets, dtype, scaler=scaler)
    have = {k for k, p in base.named_parameters() if p.grad is not None}
    crit.iter = 0
    calls = _lib.census(True)
    try:
        loss = bench.forward_backward(model, crit, NestedTensor(x.clone(), mask.clone()), text, targets, dtype, scaler=scaler)
    finally:
        _lib.census(False)
    assert torch.isfinite(loss), loss
    from ocpg_amd.models.ops.modules import MSDeformAttn
    n_mod = sum(isinstance(m_, MSDeformAttn) for m_ in model.modules())
    assert n_mod > 0 and calls.get("ocpg_msda_fwd_h16", 0) == n_mod and calls.get("ocpg_msda_bwd_h16", 0) == n_mod, calls      # every layer's op
    assert not [k for k in calls if k.startswith("ocpg_msda_") and not k.endswith("_h16")], calls
    got = {k: p.grad for k, p in model.named_parameters() if p.grad is not None}
    assert have <= set(got), sorted(have - set(got))
    bad = [k for k in have if not torch.isfinite(got[k]).all()]
    assert not bad, bad
    vp = [k for k in got if k.endswith("self_attn.value_proj.weight") or k.endswith("cross_attn.output_proj.bias")]
    assert len(vp) >= 2, vp
    for k in vp:
        assert got[k].dtype == torch.float32 and got[k].abs().max() > 0, k
    before = {k: p.detach().clone() for k, p in model.named_parameters() if p.requires_grad}
    crit.iter = 0
    opt = bench.make_optimizer(model, args, fused=False)
    step = bench.EagerStep(model, model, crit, opt, lambda: NestedTensor(x.clone(), mask.clone()), text, targets, args, dtype)
    if step.scaler is not None:
        step.scaler = torch.amp.GradScaler("cuda", init_scale=64.0)
    assert math.isfinite(float(step()))
    moved = [k for k, p in model.named_parameters() if p.requires_grad and not torch.equal(p.detach(), before[k])]
    assert set(vp) <= set(moved), sorted(set(vp) - set(moved))


def test_default_mode_has_no_16_bit_call(dev, monkeypatch):
    import bench
    from ocpg_amd import _lib
    from ocpg_amd.util.misc import NestedTensor
    monkeypatch.delenv("OCPG_MSDA_VALUE_DTYPE", raising=False)
    meta, args, model, crit = _tiny(dev)
    x, mask, targets, text = _tiny_batch(meta, dev)
    crit.iter = 0
    calls = _lib.census(True)
    try:
        loss = bench.forward_backward(model, crit, NestedTensor(x, mask), text, targets, torch.bfloat16)
    finally:
        _lib.census(False)
    assert torch.isfinite(loss)
    assert [k for k in calls if k.startswith("ocpg_msda_")] and not [k for k in calls if "_h16" in k], calls


def test_whole_step_graph_matches_eager_in_16_bit_mode(dev):
    """The scenario, assertions and tolerances of test_graph_gpu.py::test_whole_step_graph_matches_eager (bf16 leg) with
    msda_value_dtype="bf16": bench.py's GraphStep replays what the eager step computes."""
    import copy
    import bench
    from ocpg_amd.util.misc import NestedTensor
    amp = torch.bfloat16
    meta, args, model, crit = _tiny(dev, msda_value_dtype="bf16")
    det_before = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        x, mask, targets, text = _tiny_batch(meta, dev)
        make_samples = lambda: NestedTensor(x.clone(), mask.clone())
        twin, twin_crit = copy.deepcopy(model), copy.deepcopy(crit)
        n_steps = 4

        def eager_losses(m, c):
            opt = bench.make_optimizer(m, args, fused=False)
            c.iter = 0
            step = bench.EagerStep(m, m, c, opt, make_samples, text, targets, args, amp)
            return [float(step()) for _ in range(n_steps)]
        twin_crit.iter = 0
        bench.forward_backward(twin, twin_crit, make_samples(), text, targets, amp)
        g_want = {k: p.grad.clone() for k, p in twin.named_parameters() if p.grad is not None}
        twin.zero_grad(set_to_none=True)
        twin_crit.iter = 0
        bench.forward_backward(twin, twin_crit, make_samples(), text, targets, amp)
        noise = {k: (p.grad - g_want[k]).abs().max().item() for k, p in twin.named_parameters() if p.grad is not None}
        twin.zero_grad(set_to_none=True)
        want = eager_losses(twin, twin_crit)
        crit.iter = 0
        opt = bench.make_optimizer(model, args, fused=False)
        step = bench.GraphStep(model, crit, opt, make_samples, text, targets, args, amp, 1)
        assert step.memset_nodes_replaced > 0
        for rep in range(2):
            step.graph.replay()
            torch.cuda.synchronize()
            assert abs(float(step.loss) - want[0]) <= 2e-3 * abs(want[0]), (rep, float(step.loss), want[0])
            for k, p in model.named_parameters():
                if k in g_want:
                    d = (p.grad - g_want[k]).abs().max().item()
                    assert d <= 8 * noise[k] + 0.15 * g_want[k].abs().max().item() + 1e-7, (rep, k, d, noise[k])
        got = [float(step()) for _ in range(n_steps)]
    finally:
        torch.backends.cudnn.deterministic = det_before
    tol = 3e-2
    for i, (a, b) in enumerate(zip(got, want)):
        assert a == a and abs(a - b) <= tol * (1 if i < 3 else 3) * abs(b), (i, got, want)
