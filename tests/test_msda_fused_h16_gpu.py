"""Fused front end of the 16-bit MSDeformAttn value path on the GPU: ocpg_msda_fused_fwd_h16 / ocpg_msda_fused_bwd_qproj_h16,
MSDeformAttnFusedFunction with a bfloat16 / float16 value, and the module behind OCPG_MSDA_FUSED_FRONT_H16 (off by default).

Yardsticks (none of them taken from the code under test):
  loc_out / attn_out   torch's `ref + offset` / softmax in fp32, |d| <= 2e-5 max|ref| + 1e-7 (the bound of
                       test_msda_gpu.py::test_fused_front_end_equals_the_unfused_module for the same quantities)
  out                  the C oracle on the widened value at the kernel's OWN loc_out / attn_out, (u + 1e-4)|ref| + 1e-5 with u = 2^-8 / 2^-11, no
                       element exempt (_assert_forward of test_msda_h16_gpu.py)
  grad_qproj           the C oracle's grad_loc / grad_attn on the widened inputs, the softmax backward formed from them in fp64; offset half
                       <= 2e-5 max|ref|, logit half rtol 1e-3 / atol 1e-4 (the fp32 tolerances of grad_loc / grad_attn)
  module               the torch emulation and referee rule of test_module_in_16_bit_mode_vs_emulation; fused against un-fused: the fp32-mode
                       module is the yardstick and the fused path may sit at most 2x as far from it as the un-fused 16-bit path does.
"""
import math

import pytest
import torch

import test_msda_h16_gpu as h16
from cases import level_start
from test_msda_h16_gpu import CFG2, CODE, SELF_SHAPES, U, _assert_forward, _env, _local_inputs, _shifted, _ulp_at

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
IDS = ["bf16", "fp16"]
LANES = [None, "4", "8"]
LANE_IDS = ["lanes-default", "lanes4", "lanes8"]
FUSED = ("ocpg_msda_fused_fwd_h16", "ocpg_msda_bwd_value_h16", "ocpg_msda_fused_bwd_qproj_h16")


def _lanes(lanes):
    return _env(**({} if lanes is None else {"OCPG_MSDA_H16_LANES": lanes}))


def _front_inputs(N, shapes_l, dtype, M=8, D=32, P=4, seed=5):
    """_local_inputs of the existing 16-bit test, plus the fused front end's own inputs: the reference points of an encoder (every query's
    own pixel centre, the same on every level), qproj = [loc - ref | logits] and the fp32 torch results the kernel must reproduce."""
    value, shapes, ls, loc, attn, go = _local_inputs(N, shapes_l, dtype, M=M, D=D, P=P, seed=seed)
    S, L = value.shape[1], len(shapes_l)
    refs = []
    for (h, w) in shapes_l:
        ys, xs = torch.meshgrid(torch.linspace(0.5, h - 0.5, h) / h, torch.linspace(0.5, w - 0.5, w) / w, indexing="ij")
        refs.append(torch.stack([xs.reshape(-1), ys.reshape(-1)], -1))
    ref = torch.cat(refs, 0)[None, :, None, :].expand(N, S, L, 2).contiguous()
    off = loc - ref[:, :, None, :, None, :]
    g = torch.Generator().manual_seed(seed + 100)
    logits = torch.randn(N, S, M, L * P, generator=g) * 1.5
    qproj = torch.cat([off.reshape(N, S, -1), logits.reshape(N, S, -1)], -1).contiguous()
    want_loc = ref[:, :, None, :, None, :] + off
    want_attn = torch.softmax(logits, -1).view(N, S, M, L, P)
    return value, shapes, ls, qproj, ref, go, want_loc, want_attn


def _fused_fwd(dv, ds, dls, dq, dr, L, P, out=None, loc=None, attn=None, code=None):
    from ocpg_amd._lib import lib, stream_ptr
    N, S, M, D = dv.shape
    dev = dv.device
    out = torch.empty(N, S, M * D, dtype=dv.dtype, device=dev) if out is None else out
    loc = torch.empty(N, S, M, L, P, 2, device=dev) if loc is None else loc
    attn = torch.empty(N, S, M, L, P, device=dev) if attn is None else attn
    rc = lib().ocpg_msda_fused_fwd_h16(dv.data_ptr(), ds.data_ptr(), dls.data_ptr(), dq.data_ptr(), dr.data_ptr(), N, S, M, D, L, S, P,
                                       out.data_ptr(), loc.data_ptr(), attn.data_ptr(), CODE[dv.dtype] if code is None else code, stream_ptr())
    torch.cuda.synchronize()
    return rc, out, loc, attn


def _fused_gather(dv, ds, dls, dl, da, dg, gq=None, code=None):
    from ocpg_amd._lib import lib, stream_ptr
    N, S, M, D = dv.shape
    L, P = dl.shape[3], dl.shape[4]
    gq = torch.empty(N, S, 3 * M * L * P, device=dv.device) if gq is None else gq
    rc = lib().ocpg_msda_fused_bwd_qproj_h16(dv.data_ptr(), ds.data_ptr(), dls.data_ptr(), dl.data_ptr(), da.data_ptr(), dg.data_ptr(), N, S, M, D,
                                             L, S, P, gq.data_ptr(), CODE[dv.dtype] if code is None else code, stream_ptr())
    torch.cuda.synchronize()
    return rc, gq


def _assert_front(loc, attn, want_loc, want_attn, what):
    for name, got, want in (("loc", loc, want_loc), ("attn", attn, want_attn)):
        assert got.dtype == torch.float32, (what, name, got.dtype)
        d = (got.detach().cpu() - want).abs().max().item()
        tol = 2e-5 * want.abs().max().item() + 1e-7
        print(f"front end {what}: max|{name} - torch| {d:.3e} (tolerance {tol:.3e})")
        assert d <= tol, (what, name, d, tol)


def _assert_gq(gq, ogl, oga, attn, what):
    """gq [N, S, 3*M*L*P] against the oracle's grad_loc / grad_attn; the logit half through the softmax backward in fp64"""
    N, S, M, L, P = attn.shape
    n_off = 2 * M * L * P
    gq = gq.detach().cpu().view(N, S, -1)
    assert gq.dtype == torch.float32 and gq.shape[-1] == 3 * M * L * P
    a64, ga64 = attn.double().view(N, S, M, L * P), oga.double().view(N, S, M, L * P)
    want_logit = (a64 * (ga64 - (a64 * ga64).sum(-1, keepdim=True))).view(N, S, -1)
    want_off = ogl.reshape(N, S, -1)
    d_off = (gq[..., :n_off] - want_off).abs().max().item()
    d_log = (gq[..., n_off:].double() - want_logit).abs().max().item()
    print(f"fused gather {what}: offset half max|d| {d_off:.3e} (tolerance {2e-5 * want_off.abs().max().item():.3e}), "
          f"logit half max|d| {d_log:.3e}, max|ref| {want_logit.abs().max().item():.3e}")
    assert d_off <= 2e-5 * want_off.abs().max().item(), (what, d_off)
    assert torch.allclose(gq[..., n_off:], want_logit.float(), rtol=1e-3, atol=1e-4), (what, d_log)


# ---- 1. fused forward through the C ABI ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("lanes", LANES, ids=LANE_IDS)
@pytest.mark.parametrize("name", ["cfg2", "cfg5"])
def test_fused_forward_vs_torch_front_end_and_c_oracle(dev, dtype, lanes, name):
    from oracle import msda as om
    value, shapes, ls, qproj, ref, go, want_loc, want_attn = _front_inputs(1, SELF_SHAPES[name], dtype)
    dv, dq, dr, ds, dls = value.to(dev), qproj.to(dev), ref.to(dev), shapes.to(dev), ls.to(dev)
    with _lanes(lanes):
        rc, out, loc, attn = _fused_fwd(dv, ds, dls, dq, dr, 4, 4)
    assert rc == 0, rc
    _assert_front(loc, attn, want_loc, want_attn, f"{name} {lanes}")
    oc = om.msda_c_forward(value.float(), shapes, ls, loc.cpu(), attn.cpu())
    _assert_forward(out, oc, dtype, f"fused {name} lanes={lanes}")


# ---- 2. fused gather through the C ABI --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("lanes", LANES, ids=LANE_IDS)
@pytest.mark.parametrize("name", ["cfg2", "cfg5"])
def test_fused_gather_vs_c_oracle_and_bit_reproducible(dev, dtype, lanes, name):
    from oracle import msda as om
    value, shapes, ls, loc, attn, go = _local_inputs(1, SELF_SHAPES[name], dtype, seed=6)
    _, ogl, oga = om.msda_c_backward(value.float(), shapes, ls, loc, attn, go.float())
    dv, dl, da, dg, ds, dls = value.to(dev), loc.to(dev), attn.to(dev), go.to(dev), shapes.to(dev), ls.to(dev)
    with _lanes(lanes):
        rc, gq = _fused_gather(dv, ds, dls, dl, da, dg)
        rc2, gq2 = _fused_gather(dv, ds, dls, dl, da, dg, gq=torch.full_like(gq, 3.0))
    assert rc == 0 and rc2 == 0, (rc, rc2)
    _assert_gq(gq, ogl, oga, attn, f"{name} lanes={lanes}")
    assert torch.equal(gq, gq2)                 # no atomics on this side: the same bits, every element overwritten


# ---- 3. argument contract ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_declined_shapes_and_dtype_codes_launch_nothing(dev, dtype):
    cases_ = {"D=16": dict(shapes_l=[(16, 24), (8, 12), (4, 6), (2, 3)], M=4, D=16, P=4), "L*P=12": dict(shapes_l=SELF_SHAPES["cfg1_3lvl"], M=8, D=32, P=4)}
    for what, kw in cases_.items():
        shapes_l = kw.pop("shapes_l")
        L, P = len(shapes_l), kw["P"]
        value, shapes, ls, qproj, ref, go, want_loc, want_attn = _front_inputs(1, shapes_l, dtype, **kw)
        dv, dq, dr, ds, dls = value.to(dev), qproj.to(dev), ref.to(dev), shapes.to(dev), ls.to(dev)
        N, S, M, D = value.shape
        out = torch.full((N, S, M * D), 7.0, device=dev).to(dtype)
        loc, attn = torch.full((N, S, M, L, P, 2), 7.0, device=dev), torch.full((N, S, M, L, P), 7.0, device=dev)
        rc, *_ = _fused_fwd(dv, ds, dls, dq, dr, L, P, out, loc, attn)
        assert rc == -2000, (what, rc)
        assert (out.float() == 7.0).all() and (loc == 7.0).all() and (attn == 7.0).all(), what
        gq = torch.full((N, S, 3 * M * L * P), 7.0, device=dev)
        rc, _ = _fused_gather(dv, ds, dls, want_loc.to(dev).contiguous(), want_attn.to(dev).contiguous(), go.to(dev), gq=gq)
        assert rc == -2000 and (gq == 7.0).all(), (what, rc)
    # an unknown dtype code: the invalid-argument status of the symbol, nothing written
    value, shapes, ls, qproj, ref, go, want_loc, want_attn = _front_inputs(1, [(8, 12), (4, 6), (2, 3), (1, 2)], dtype)
    dv, dq, dr, ds, dls = value.to(dev), qproj.to(dev), ref.to(dev), shapes.to(dev), ls.to(dev)
    N, S, M, D = value.shape
    for code in (0, 3):
        out = torch.full((N, S, M * D), 7.0, device=dev).to(dtype)
        loc, attn = torch.full((N, S, M, 4, 4, 2), 7.0, device=dev), torch.full((N, S, M, 4, 4), 7.0, device=dev)
        rc, *_ = _fused_fwd(dv, ds, dls, dq, dr, 4, 4, out, loc, attn, code=code)
        assert rc == -1016, (code, rc)
        assert (out.float() == 7.0).all() and (loc == 7.0).all() and (attn == 7.0).all(), code
        gq = torch.full((N, S, 3 * M * 16), 7.0, device=dev)
        rc, _ = _fused_gather(dv, ds, dls, want_loc.to(dev).contiguous(), want_attn.to(dev).contiguous(), go.to(dev), gq=gq, code=code)
        assert rc == -1015 and (gq == 7.0).all(), (code, rc)
    # the same small problem with a valid code is served (the statuses above are about the code, not the shape)
    rc, out, loc, attn = _fused_fwd(dv, ds, dls, dq, dr, 4, 4)
    assert rc == 0
    _assert_front(loc, attn, want_loc, want_attn, "small")


class _ShiftedGrad(torch.autograd.Function):
    """identity whose backward hands on a contiguous copy of the gradient that sits 2 bytes past a 16-byte boundary"""

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return _shifted(g.contiguous(), 2)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("which", ["value", "grad_out"])
def test_buffer_off_the_16_byte_boundary(dev, dtype, which):
    """The symbol that reads the shifted buffer answers -2000 and writes nothing; MSDeformAttnFusedFunction still returns results within the
    bounds of the tests above (un-fused 16-bit entry points, front end / softmax backward in torch)."""
    from oracle import msda as om
    from ocpg_amd import _lib
    from ocpg_amd.models.ops.functions.ms_deform_attn_func import MSDeformAttnFusedFunction
    shapes_l = [(16, 24), (8, 12), (4, 6), (2, 3)]
    value, shapes, ls, qproj, ref, go, want_loc, want_attn = _front_inputs(1, shapes_l, dtype, seed=8)
    dv, dq, dr, dg, ds, dls = value.to(dev), qproj.to(dev), ref.to(dev), go.to(dev), shapes.to(dev), ls.to(dev)
    ds._ocpg_host = shapes
    N, S, M, D = value.shape
    if which == "value":
        dv = _shifted(dv, 8)
        out = torch.full((N, S, M * D), 7.0, device=dev).to(dtype)
        loc, attn = torch.full((N, S, M, 4, 4, 2), 7.0, device=dev), torch.full((N, S, M, 4, 4), 7.0, device=dev)
        rc, *_ = _fused_fwd(dv, ds, dls, dq, dr, 4, 4, out, loc, attn)
        assert rc == -2000 and (out.float() == 7.0).all() and (loc == 7.0).all() and (attn == 7.0).all(), rc
    gq = torch.full((N, S, 3 * M * 16), 7.0, device=dev)
    rc, _ = _fused_gather(dv, ds, dls, want_loc.to(dev).contiguous(), want_attn.to(dev).contiguous(),
                          _shifted(dg, 2) if which == "grad_out" else dg, gq=gq)
    assert rc == -2000 and (gq == 7.0).all(), rc
    # through the autograd function
    v, q = dv.detach().requires_grad_(True), dq.clone().requires_grad_(True)
    state = torch.zeros(8, dtype=torch.int32, device=dev)
    calls = _lib.census(True)
    try:
        out, loc, attn = MSDeformAttnFusedFunction.apply(v, ds, dls, q, dr, 4, 4, state)
        o = _ShiftedGrad.apply(out) if which == "grad_out" else out
        o.backward(dg)
    finally:
        _lib.census(False)
    print(f"shifted {which}: {calls}")
    if which == "value":
        assert calls.get("ocpg_msda_fwd_h16") == 1 and "ocpg_msda_fused_fwd_h16" not in calls, calls
    else:
        assert calls.get("ocpg_msda_fused_fwd_h16") == 1, calls
    assert calls.get("ocpg_msda_bwd_h16") == 1 and "ocpg_msda_fused_bwd_qproj_h16" not in calls, calls
    assert out.dtype == dtype and v.grad.dtype == dtype and q.grad.dtype == torch.float32
    _assert_front(loc, attn, want_loc, want_attn, f"shifted {which}")
    oc = om.msda_c_forward(value.float(), shapes, ls, loc.cpu(), attn.cpu())
    _assert_forward(out.detach(), oc, dtype, f"shifted {which}")
    ogv, ogl, oga = om.msda_c_backward(value.float(), shapes, ls, loc.cpu(), attn.cpu(), go.float())
    _assert_gq(q.grad, ogl, oga, attn.cpu(), f"shifted {which}")
    err16 = (v.grad.float().cpu() - ogv).abs()          # the fp32 result rounded once: _assert_backward's bound for the 16-bit grad_value
    assert (err16 <= (U[dtype] + 1e-4 + 1e-3) * ogv.abs() + 1e-4 + 1e-5).all(), (err16 / (ogv.abs() + 1e-4)).max().item()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_autograd_function_dtypes_and_gradients_vs_c_oracle(dev, dtype):
    """MSDeformAttnFusedFunction on aligned buffers: the three fused-path symbols once each, out / grad_value in value's dtype, loc / attn /
    grad_qproj fp32, gradients within the bounds of the C-ABI tests; a grad_output of another dtype is refused."""
    from oracle import msda as om
    from ocpg_amd import _lib
    from ocpg_amd.models.ops.functions.ms_deform_attn_func import MSDeformAttnFusedFunction
    value, shapes, ls, qproj, ref, go, want_loc, want_attn = _front_inputs(1, CFG2, dtype, seed=9)
    dv, dq, dr, dg, ds, dls = value.to(dev), qproj.to(dev), ref.to(dev), go.to(dev), shapes.to(dev), ls.to(dev)
    ds._ocpg_host = shapes
    assert MSDeformAttnFusedFunction.supported(dv, dq, dr, 4, 4)
    v, q = dv.clone().requires_grad_(True), dq.clone().requires_grad_(True)
    state = torch.zeros(8, dtype=torch.int32, device=dev)
    calls = _lib.census(True)
    try:
        out, loc, attn = MSDeformAttnFusedFunction.apply(v, ds, dls, q, dr, 4, 4, state)
        out.backward(dg)
    finally:
        _lib.census(False)
    assert {k: calls.get(k) for k in FUSED} == {k: 1 for k in FUSED} and len(calls) == 3, calls
    assert int(state[7]) > 0
    assert out.dtype == dtype and loc.dtype == torch.float32 and attn.dtype == torch.float32
    assert v.grad.dtype == dtype and q.grad.dtype == torch.float32 and q.grad.shape == q.shape
    _assert_front(loc, attn, want_loc, want_attn, "function")
    ogv, ogl, oga = om.msda_c_backward(value.float(), shapes, ls, loc.cpu(), attn.cpu(), go.float())
    _assert_gq(q.grad, ogl, oga, attn.cpu(), "function")
    err16 = (v.grad.float().cpu() - ogv).abs()
    assert (err16 <= (U[dtype] + 1e-4 + 1e-3) * ogv.abs() + 1e-4 + 1e-5).all(), (err16 / (ogv.abs() + 1e-4)).max().item()
    with pytest.raises(RuntimeError, match="grad_output must have value's dtype"):
        MSDeformAttnFusedFunction._backward_h16(_Ctx(q.shape), dv, ds, dls, loc, attn, dg.float(), shapes)


class _Ctx:
    def __init__(self, qshape):
        self.qshape, self.sel_state = qshape, None


# ---- 4., 5., 7. the module --------------------------------------------------------------------------------------------------------
def _module_case(dev, pad, N=2):
    """Inputs and trained-looking projections of test_module_in_16_bit_mode_vs_emulation (config-#2 encoder shape)."""
    from ocpg_amd.models.ops.modules import MSDeformAttn
    shapes, ls = level_start(CFG2)
    S = int(shapes.prod(1).sum())
    g = torch.Generator().manual_seed(11)
    torch.manual_seed(11)
    m = MSDeformAttn(256, 4, 8, 4)
    with torch.no_grad():
        m.sampling_offsets.weight.copy_(torch.randn(m.sampling_offsets.weight.shape, generator=g) * 0.05)
        m.attention_weights.weight.copy_(torch.randn(m.attention_weights.weight.shape, generator=g) * 0.2)
        m.attention_weights.bias.copy_(torch.randn(m.attention_weights.bias.shape, generator=g) * 0.5)
    refs = []
    for (h, w) in CFG2:
        ys, xs = torch.meshgrid((torch.arange(h) + 0.5) / h, (torch.arange(w) + 0.5) / w, indexing="ij")
        refs.append(torch.stack([xs.reshape(-1), ys.reshape(-1)], -1))
    ref = torch.cat(refs, 0)[None, :, None, :].expand(N, S, 4, 2).contiguous().to(dev)
    q = torch.randn(N, S, 256, generator=g).to(dev)
    src = torch.randn(N, S, 256, generator=g).to(dev)
    go = torch.randn(N, S, 256, generator=g).to(dev)
    mask = None
    if pad:
        mask = torch.zeros(N, S, dtype=torch.bool)
        mask[1, 3000:3600] = True
        mask = mask.to(dev)
    ds, dls = shapes.to(dev), ls.to(dev)
    ds._ocpg_host = shapes
    return m.state_dict(), (q, ref, src, ds, dls, mask, go), shapes


def _run_module(dev, monkeypatch, state, inputs, value_dtype, fused):
    """one forward + backward of a fresh module with the given weights -> (module, out, loc, attn, grads by name, census)"""
    from ocpg_amd import _lib
    from ocpg_amd.models.ops.modules import MSDeformAttn
    from ocpg_amd.models.ops.modules import ms_deform_attn as mod_file
    monkeypatch.setattr(mod_file, "FUSED_FRONT_H16", fused)
    q, ref, src, ds, dls, mask, go = inputs
    m = MSDeformAttn(256, 4, 8, 4, value_dtype=value_dtype)
    m.load_state_dict(state)
    m.to(dev)
    q, src = q.clone().requires_grad_(True), src.clone().requires_grad_(True)
    names = ["query", "source"] + [k for k, _ in m.named_parameters()]
    calls = _lib.census(True)
    try:
        out, loc, attn = m(q, ref, src, ds, dls, mask)
        grads = torch.autograd.grad((out.float() * go).sum(), [q, src] + list(m.parameters()))
    finally:
        _lib.census(False)
    return m, out, loc, attn, dict(zip(names, grads)), dict(calls), src


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("pad", [False, True], ids=["nopad", "pad"])
def test_module_with_the_switch_on_vs_emulation(dev, monkeypatch, dtype, pad):
    import torch.nn.functional as F
    from oracle.msda import msda_torch
    state, inputs, shapes = _module_case(dev, pad)
    m, out, loc, attn, grads, calls, src = _run_module(dev, monkeypatch, state, inputs, dtype, True)
    _, _, _, _, grads_unfused, calls_unfused, _ = _run_module(dev, monkeypatch, state, inputs, dtype, False)
    mask = inputs[5]
    N, S = src.shape[:2]
    assert {k: calls.get(k) for k in FUSED} == {k: 1 for k in FUSED}, calls
    assert "ocpg_msda_fwd_h16" not in calls and "ocpg_msda_bwd_h16" not in calls, calls
    assert not [k for k in calls if k.startswith("ocpg_msda_") and not k.endswith("_h16")], calls
    assert out.dtype == dtype and loc.dtype == torch.float32 and attn.dtype == torch.float32
    assert int(m._sel_state[7]) > 0
    for k, g_ in grads.items():
        assert torch.isfinite(g_).all(), k
        if grads_unfused[k].abs().max() > 0:
            assert g_.abs().max() > 0, k
    assert grads["query"].abs().max() > 0 and grads["source"].abs().max() > 0

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
    print(f"fused module ({dtype}, pad={pad}): max|module - emulation| {d_mod:.3e}; referee: max|emulation - fp64 emulation| {d_ref:.3e}; "
          f"max|out| {mx:.3f}, one ulp there {_ulp_at(mx, dtype):.3e}, tolerance {tol:.3e}")
    assert d_mod <= tol, (d_mod, d_ref, tol)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("lanes", LANES, ids=LANE_IDS)
def test_fused_vs_unfused_16_bit_module_against_the_fp32_module(dev, monkeypatch, dtype, lanes):
    """Same build, same weights, same inputs: the fp32-mode module is the yardstick; the fused 16-bit path may be at most twice as far
    from it as the un-fused 16-bit path (same cast points, so equal distances are expected; 2x covers the spread of a max-norm)."""
    state, inputs, _ = _module_case(dev, True)
    with _lanes(lanes):
        _, out_f, loc_f, attn_f, g_f, calls_f, _ = _run_module(dev, monkeypatch, state, inputs, dtype, True)
        _, out_u, loc_u, attn_u, g_u, calls_u, _ = _run_module(dev, monkeypatch, state, inputs, dtype, False)
    _, out_0, loc_0, attn_0, g_0, calls_0, _ = _run_module(dev, monkeypatch, state, inputs, None, True)
    assert calls_f.get("ocpg_msda_fused_fwd_h16") == 1 and calls_u.get("ocpg_msda_fwd_h16") == 1 and "ocpg_msda_fused_fwd_h16" not in calls_u
    assert not [k for k in calls_0 if "_h16" in k], calls_0
    for name, a, b in (("loc", loc_f, loc_u), ("attn", attn_f, attn_u)):
        d = (a - b).abs().max().item()
        tol = 2e-5 * b.abs().max().item() + 1e-7
        print(f"fused vs un-fused ({dtype}, lanes={lanes}) {name}: max|d| {d:.3e} (tolerance {tol:.3e})")
        assert d <= tol, (name, d, tol)
    rows = [("out", out_f, out_u, out_0)] + [(k, g_f[k], g_u[k], g_0[k]) for k in g_0]
    bad = []
    for name, f, u, z in rows:
        d_f = (f.detach().double() - z.detach().double()).abs().max().item()
        d_u = (u.detach().double() - z.detach().double()).abs().max().item()
        print(f"distance from the fp32 module ({dtype}, lanes={lanes}) {name}: fused {d_f:.4e}, un-fused {d_u:.4e}, max|fp32| {z.abs().max().item():.4e}")
        if not d_f <= 2.0 * d_u:
            bad.append((name, d_f, d_u))
    assert not bad, bad


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_switch_off_keeps_the_un_fused_census(dev, monkeypatch, dtype):
    state, inputs, _ = _module_case(dev, False)
    m, out, loc, attn, grads, calls, _ = _run_module(dev, monkeypatch, state, inputs, dtype, False)
    assert calls.get("ocpg_msda_fwd_h16") == 1 and calls.get("ocpg_msda_bwd_h16") == 1, calls
    assert not [k for k in calls if "fused" in k], calls
    assert not [k for k in calls if k.startswith("ocpg_msda_") and not k.endswith("_h16")], calls
    assert int(m._sel_state[7]) > 0


def test_switch_is_off_in_this_process_unless_the_variable_says_so():
    import os
    from ocpg_amd.models.ops.modules import ms_deform_attn as mod_file
    assert mod_file.FUSED_FRONT_H16 == (os.environ.get("OCPG_MSDA_FUSED_FRONT_H16", "0") != "0")


# ---- 6. end to end ------------------------------------------------------------------------------------------------------------------
def _tiny_d32(dev, fixture="e2e_d32", **over):
    """The tiny end-to-end model at head dimension 32 (hidden 64 / 2 heads: the encoder's self-attention qualifies for the fused front end).
    e2e_d32: the committed ResNet fixture as it is.  e2e_swin: the committed tiny Video-Swin fixture's configuration and inputs with
    nheads = 2; its weights come from the same generator, for the shapes this model has."""
    import cases
    import model_checks
    import synth
    from conftest import Golden
    meta = Golden(fixture).meta
    if "swin_cfg" in meta:
        from ocpg_amd.models import build_model
        args = cases.default_args(device=str(dev), video_swin_cfg=meta["swin_cfg"], **meta["cfg"], nheads=2, **over)
        model, crit, _ = build_model(args)
        shapes = {k: tuple(v.shape) for k, v in model.state_dict().items() if v.dtype.is_floating_point}
        missing = model.load_state_dict(synth.synth_state_dict(shapes, seed=meta["seed"]), strict=False)
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


def _tiny_batch_d32(meta, dev):
    import cases
    import model_checks
    B, T, H, W = meta.get("B", 2), meta["T"], meta["H"], meta["W"]
    x, mask, targets = cases.e2e_inputs(B, T, H, W, meta["pad_sizes"], dev)
    return x, mask, targets, model_checks.text_for(B, dev)


def _enc_dec(model):
    from ocpg_amd.models.ops.modules import MSDeformAttn
    names = [k for k, m_ in model.named_modules() if isinstance(m_, MSDeformAttn)]
    enc = [k for k in names if ".encoder." in k]
    return len(enc), len(names) - len(enc)


@pytest.mark.parametrize("dtype,word", [(torch.bfloat16, "bf16"), (torch.float16, "fp16")], ids=["bf16", "fp16"])
def test_tiny_training_step_with_the_switch_on(dev, monkeypatch, dtype, word):
    """test_tiny_training_step_in_16_bit_mode with OCPG_MSDA_FUSED_FRONT_H16 on, on fixtures whose encoder qualifies (head dimension 32):
    every encoder layer runs the three fused-path symbols, every decoder layer the un-fused 16-bit op."""
    import bench
    from ocpg_amd import _lib
    from ocpg_amd.models.ops.modules import ms_deform_attn as mod_file
    from ocpg_amd.util.misc import NestedTensor
    monkeypatch.setattr(mod_file, "FUSED_FRONT_H16", True)
    fixture = "e2e_swin" if dtype == torch.float16 else "e2e_d32"
    meta, args, model, crit = _tiny_d32(dev, fixture, msda_value_dtype=word)
    _, _, base, base_crit = _tiny_d32(dev, fixture)
    x, mask, targets, text = _tiny_batch_d32(meta, dev)
    scaler = torch.amp.GradScaler("cuda", init_scale=64.0) if dtype == torch.float16 else None
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
    n_enc, n_dec = _enc_dec(model)
    assert n_enc > 0 and n_dec > 0
    for k in FUSED:
        assert calls.get(k, 0) == n_enc, (k, calls)
    assert calls.get("ocpg_msda_fwd_h16", 0) == n_dec and calls.get("ocpg_msda_bwd_h16", 0) == n_dec, calls
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


def test_whole_step_graph_matches_eager_with_the_switch_on(dev, monkeypatch):
    """The scenario, assertions and tolerances of test_whole_step_graph_matches_eager_in_16_bit_mode, run as they stand on the head-dimension-32
    fixture with the fused 16-bit front end on; the census of the capture shows the fused symbols."""
    from ocpg_amd import _lib
    from ocpg_amd.models.ops.modules import ms_deform_attn as mod_file
    monkeypatch.setattr(mod_file, "FUSED_FRONT_H16", True)
    monkeypatch.setattr(h16, "_tiny", lambda dev_, fixture="e2e_d32", **over: _tiny_d32(dev_, "e2e_d32", **over))
    monkeypatch.setattr(h16, "_tiny_batch", _tiny_batch_d32)
    calls = _lib.census(True)
    try:
        h16.test_whole_step_graph_matches_eager_in_16_bit_mode(dev)
    finally:
        _lib.census(False)
    for k in FUSED:
        assert calls.get(k, 0) > 0, (k, calls)
    assert not [k for k in calls if k.startswith("ocpg_msda_") and not k.endswith("_h16")], calls
