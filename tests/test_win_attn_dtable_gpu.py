"""The opt-in window-attention backward that returns the gradient of the relative-position TABLE (csrc/win_attn_mfma.hip, DTABLE;
`window_attention_table`): against fp32 autograd of the tensor-op formulation on the same rounded inputs, with the un-fused matrix-core
path (`window_attention` + `RelPosBias`: dS tensor, ATen sum, relpos_bias_bwd) as the yardstick; unused table rows; the path taken
when the table needs no gradient; the reference's own vectors through the model code; graph replay."""
import ctypes

import pytest
import torch

import swin_checks
from test_win_attn_gpu import _reference

pytestmark = pytest.mark.gpu

SHAPES = [(6, 3, 245, 3, True, (8, 7, 7)), (4, 2, 392, 4, True, (8, 7, 7)), (4, 4, 245, 6, False, (8, 7, 7)), (3, 1, 37, 2, True, (8, 7, 7)),
          (5, 1, 98, 2, True, (2, 7, 7))]
_DT = {torch.bfloat16: 1, torch.float16: 2}


def _inputs(dev, dtype, bw, nw, n, h, shift, window):
    """Index of a real WindowAttention3D, table randn * 0.5, the rest as tests/test_win_attn_gpu.py generates it."""
    import ocpg_amd.models.video_swin_transformer as vs
    wa = vs.WindowAttention3D(32 * h, window, h).to(dev)
    idx2 = wa.relative_position_index[:n, :n]
    g = torch.Generator(device=dev).manual_seed(n * 7 + h)
    qkv = torch.randn(bw, n, 3, h, 32, device=dev, generator=g).to(dtype)
    table = torch.randn(wa.relative_position_bias_table.shape, device=dev, generator=g) * 0.5
    region = (torch.randint(0, 3, (nw, n), device=dev, generator=g).int() if shift else None)
    go = torch.randn(bw, n, h * 32, device=dev, generator=g)
    return idx2, qkv, table, region, go, 32 ** -0.5


def _unfused(qkv, table, idx2, region, scale, nw):
    """Today's default path of the model: RelPosBias (both layouts, one launch) + window_attention."""
    from ocpg_amd.models.ops.functions.layernorm_func import RelPosBias, StaticGather
    from ocpg_amd.models.ops.functions.win_attn_func import window_attention
    bias, bias_t = RelPosBias.apply(table, idx2, StaticGather.plan(idx2.reshape(-1), table.shape[0]))
    return window_attention(qkv, bias, region, scale, nw, bias_t)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("bw,nw,n,h,shift,window", SHAPES)
def test_fused_table_gradient(dev, dtype, bw, nw, n, h, shift, window):
    from ocpg_amd.models.ops.functions.win_attn_func import window_attention_table
    idx2, qkv, table, region, go, scale = _inputs(dev, dtype, bw, nw, n, h, shift, window)
    # fp32 reference on the SAME (rounded) inputs
    a = qkv.float().requires_grad_(True)
    tb = table.clone().requires_grad_(True)
    want = _reference(a, tb[idx2.reshape(-1)].view(n, n, h).permute(2, 0, 1), region, scale, nw)
    want_gx, want_gt = torch.autograd.grad((want * go).sum(), (a, tb))
    res = []
    for fn in (_unfused, window_attention_table):
        x, t = qkv.clone().requires_grad_(True), table.clone().requires_grad_(True)
        out = fn(x, t, idx2, region, scale, nw)
        gx, gt = torch.autograd.grad((out.float() * go).sum(), (x, t))
        assert gt.shape == table.shape and gt.dtype == torch.float32
        res.append((out, gx, gt))
    (out_old, gx_old, gt_old), (out_new, gx_new, gt_new) = res
    assert torch.equal(out_new, out_old)                  # the same forward kernel
    eps = 2 ** -8 if dtype == torch.bfloat16 else 2 ** -11
    if dtype == torch.bfloat16:
        assert torch.equal(gx_new, gx_old)                # no atomics touch dqkv: the two instantiations compute it alike
    else:
        # fp16: hipcc rounds the plain kernel's dS operand ONCE (v_fma_mixlo_f16: product and conversion in one instruction); the
        # variant needs the fp32 product for the table and converts that, so dS can differ in its last bit.  dqkv is therefore held to
        # the bound of tests/test_win_attn_gpu.py against fp32, with the un-fused path as the yardstick.
        scale_x = want_gx.abs().max().item()
        ex_new, ex_old = (gx_new.float() - want_gx).abs().max().item(), (gx_old.float() - want_gx).abs().max().item()
        print("dqkv %s n %d: e_new %.3e e_old %.3e max|ref| %.3e" % (dtype, n, ex_new, ex_old, scale_x))
        assert ex_new <= 1.5 * ex_old + 6 * eps * scale_x, (ex_new, ex_old, scale_x)
    scale_v = want_gt.abs().max().item()
    e_new, e_old = (gt_new - want_gt).abs().max().item(), (gt_old - want_gt).abs().max().item()
    print("dtable %s n %d: e_new %.3e e_old %.3e max|ref| %.3e" % (dtype, n, e_new, e_old, scale_v))
    assert e_new <= 1.5 * e_old + 6 * eps * scale_v, (e_new, e_old, scale_v)


def test_unused_table_rows_are_exact_zeros(dev):
    """Raw ABI, partials and dtable pre-filled with NaN: an un-zeroed LDS table, an un-written partial, or a padded query / key that
    leaks in would show as a non-finite value or in one of the 1014 rows the clamped window never addresses."""
    from ocpg_amd._lib import check, lib, stream_ptr
    from ocpg_amd.models.ops.functions.win_attn_func import table_codes
    bw, nw, n, h, shift, window = SHAPES[0]
    dtype = torch.bfloat16
    idx2, qkv, table, region, go, scale = _inputs(dev, dtype, bw, nw, n, h, shift, window)
    rows = table.shape[0]
    code, off = table_codes(idx2)
    assert lib().ocpg_win_attn_dtable_supported(n, 32, _DT[dtype], rows) == 1
    bias, bias_t = torch.empty(h, n, n, device=dev), torch.empty(h, n, n, device=dev)
    out, lse = torch.empty(bw, n, h * 32, dtype=dtype, device=dev), torch.empty(bw, h, n, device=dev)
    check(lib().ocpg_relpos_bias_fwd(table.data_ptr(), idx2.data_ptr(), n, idx2.stride(0), h, bias.data_ptr(), bias_t.data_ptr(), stream_ptr()),
          "ocpg_relpos_bias_fwd")
    check(lib().ocpg_win_attn_fwd(qkv.data_ptr(), bias_t.data_ptr(), region.data_ptr(), scale, bw, nw, n, h, 32, out.data_ptr(), lse.data_ptr(),
                                  _DT[dtype], stream_ptr()), "ocpg_win_attn_fwd")
    dout = go.to(dtype)
    dqkv, dbuf = torch.empty_like(qkv), torch.empty_like(lse)
    partials = torch.full((bw, h, rows), float("nan"), device=dev)
    dtable = torch.full((rows, h), float("nan"), device=dev)
    check(lib().ocpg_win_attn_bwd_mfma_dtable(qkv.data_ptr(), bias.data_ptr(), bias_t.data_ptr(), region.data_ptr(), scale, bw, nw, n, h, 32,
                                              out.data_ptr(), dout.data_ptr(), lse.data_ptr(), dqkv.data_ptr(), dbuf.data_ptr(),
                                              code.data_ptr(), off, rows, partials.data_ptr(), dtable.data_ptr(), _DT[dtype], stream_ptr()),
          "ocpg_win_attn_bwd_mfma_dtable")
    assert torch.isfinite(dtable).all() and torch.isfinite(partials).all() and torch.isfinite(dqkv.float()).all()
    used = torch.zeros(rows, dtype=torch.bool, device=dev)
    used[idx2.reshape(-1)] = True
    assert int(used.sum()) == 1521 and rows == 2535
    assert (dtable[~used] == 0).all() and (partials[:, :, ~used] == 0).all()
    assert (dtable[used] != 0).any(1).float().mean().item() > 0.99       # (a corner row has one pair per window: it can be masked to 0)
    # a shape outside the kernel's LDS is refused before anything is launched
    assert lib().ocpg_win_attn_dtable_supported(n, 32, _DT[dtype], 40000) == 0
    assert lib().ocpg_win_attn_dtable_supported(n, 32, 0, rows) == 0 and lib().ocpg_win_attn_dtable_supported(n, 64, _DT[dtype], rows) == 0
    dtable.fill_(float("nan"))
    rc = lib().ocpg_win_attn_bwd_mfma_dtable(qkv.data_ptr(), bias.data_ptr(), bias_t.data_ptr(), region.data_ptr(), scale, bw, nw, n, h, 32,
                                             out.data_ptr(), dout.data_ptr(), lse.data_ptr(), dqkv.data_ptr(), dbuf.data_ptr(),
                                             code.data_ptr(), off, 40000, partials.data_ptr(), dtable.data_ptr(), _DT[dtype], stream_ptr())
    assert rc == -2000 and torch.isnan(dtable).all()


def test_table_without_gradient_takes_the_existing_backward(dev):
    from ocpg_amd import _lib
    from ocpg_amd.models.ops.functions.win_attn_func import window_attention_table
    bw, nw, n, h, shift, window = SHAPES[0]
    idx2, qkv, table, region, go, scale = _inputs(dev, torch.bfloat16, bw, nw, n, h, shift, window)
    x0 = qkv.clone().requires_grad_(True)
    gx_default, = torch.autograd.grad((_unfused(x0, table, idx2, region, scale, nw).float() * go).sum(), x0)
    x = qkv.clone().requires_grad_(True)
    c = _lib.census(True)
    try:
        out = window_attention_table(x, table, idx2, region, scale, nw)
        gx, = torch.autograd.grad((out.float() * go).sum(), x)
    finally:
        _lib.census(False)
    assert c.get("ocpg_win_attn_bwd_mfma", 0) == 1 and "ocpg_win_attn_bwd_mfma_dtable" not in c, c
    assert torch.equal(gx, gx_default)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("check,fixture", [("check_window_attention_16bit", "swin3d"), ("check_window_attention_n392", "swin_n392")])
def test_reference_vectors_through_the_model_switch(golden, dev, monkeypatch, dtype, check, fixture):
    """WindowAttention3D with the switch on, on the reference's own vectors (table gradient included) within the existing 16-bit bounds;
    the census proves which backward served it."""
    import ocpg_amd.models.video_swin_transformer as vs
    from ocpg_amd import _lib
    monkeypatch.setattr(vs, "_FUSED_DTABLE", True)
    c = _lib.census(True)
    try:
        getattr(swin_checks, check)(golden(fixture), dev, dtype)
    finally:
        _lib.census(False)
    assert c.get("ocpg_win_attn_bwd_mfma_dtable", 0) == 2, c
    assert not {"ocpg_win_attn_bwd_mfma", "ocpg_win_attn_bwd", "ocpg_relpos_bias_bwd"} & set(c), c


def test_graph_replay(dev):
    """Forward + backward of one attention captured once, replayed on two sets of static inputs: each replay's table gradient agrees
    with an eager run to the fp32 sum-order bound (only the order of the LDS adds varies), and the capture holds no memset node
    (partials and dtable are fully written, never zeroed)."""
    from ocpg_amd import _lib
    from ocpg_amd.models.ops.functions.win_attn_func import table_codes, window_attention_table
    bw, nw, n, h, window, dtype = 4, 2, 245, 3, (8, 7, 7), torch.bfloat16
    idx2, qkv, table, region, go, scale = _inputs(dev, dtype, bw, nw, n, h, True, window)
    codes = table_codes(idx2)                                # (a device round trip: before the capture)
    xs, gos = qkv.clone().requires_grad_(True), go.to(dtype)
    tb = table.clone().requires_grad_(True)

    def step():
        out = window_attention_table(xs, tb, idx2, region, scale, nw, codes)
        return torch.autograd.grad(out, (xs, tb), gos)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(graph, stream=side):
        gx_s, gt_s = step()
    st = (ctypes.c_longlong * 9)()
    _lib.check(_lib.lib().ocpg_graph_stats(graph.raw_cuda_graph(), st), "ocpg_graph_stats")
    assert st[6] == 0 and st[5] >= 5, list(st)             # no memset node; relpos, fwd, bwd_q, reduce, bwd_kv kernels
    graph.instantiate()
    g = torch.Generator(device=dev).manual_seed(99)
    for r in range(2):
        with torch.no_grad():
            xs.copy_(torch.randn(xs.shape, device=dev, generator=g).to(dtype))
            gos.copy_(torch.randn(gos.shape, device=dev, generator=g).to(dtype))
            gt_s.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        got_x, got_t = gx_s.clone(), gt_s.clone()
        ref_x, ref_t = step()
        assert torch.equal(got_x, ref_x), r
        assert (got_t - ref_t).abs().max().item() <= 2e-5 * ref_t.abs().max().item() + 1e-6, r
