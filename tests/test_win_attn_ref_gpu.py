"""Every window-attention path (csrc/win_attn.hip, csrc/win_attn_mfma.hip) against the fp64 reference of tests/win_attn_ref.py, each
output element held to the bound derived there: |got - ref| <= bound, no multiplier, no max|ref|, no other kernel as the yardstick
(tests/test_win_attn_bounds_cpu.py shows what this harness sees and what it does not).

(a) out, lse, dqkv and dbias / dtable of every case through: fp32 (vector-ALU kernels), bf16 / fp16 on the matrix cores (dS + sum),
    bf16 / fp16 with OCPG_WIN_ATTN_MFMA=0 (vector-ALU kernels), bf16 / fp16 through `window_attention_table`; the census proves which
    backward served the call.  The cases: N = 1, 31, 32, 33, 64, 65, 129 around the 32-wide tiles, region rows that are uniform while
    `region` is non-null, a masked key that carries all the weight of a row (-100 is finite), peaked softmaxes, no region, BW = 1.
(b) Through the raw ABI with every output a slice of a larger buffer: payloads pre-filled with NaN (dbiasT with zeros) come back
    finite -- no element of a padded tile left un-written -- and the guard bands around them keep their sentinel bits: no write past N.
(c) The pre-transposed `bias_t` argument changes no bit.

c32 = 16 for the fp32 kernels held on the MI355X (v_exp_f32 / v_log_f32 behind __expf / __logf): the worst measured ratios are in
DESIGN.md section 4.5.
"""
import pytest
import torch

import win_attn_ref as wr

pytestmark = pytest.mark.gpu

_DT = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}
WINDOW = (8, 7, 7)
GUARD = 4096
PATHS = [("valu", torch.float32), ("mfma", torch.bfloat16), ("mfma", torch.float16), ("valu", torch.bfloat16), ("valu", torch.float16),
         ("table", torch.bfloat16), ("table", torch.float16)]
PATH_IDS = ["%s-%s" % (p, str(d).split(".")[1]) for p, d in PATHS]
_INDEX = []
_BWD_ENTRY = {"valu": "ocpg_win_attn_bwd", "mfma": "ocpg_win_attn_bwd_mfma", "table": "ocpg_win_attn_bwd_mfma_dtable"}


def _real_index(n):
    """relative_position_index[:n, :n] of a real WindowAttention3D (a view with the full row stride, as the model passes it)."""
    if not _INDEX:
        import ocpg_amd.models.video_swin_transformer as vs
        _INDEX.append(vs.WindowAttention3D(32, WINDOW, 1).relative_position_index)
        assert torch.equal(_INDEX[0], wr.swin_index(WINDOW))
    return _INDEX[0][:n, :n]


def _set_path(monkeypatch, path):
    if path == "valu":
        monkeypatch.setenv("OCPG_WIN_ATTN_MFMA", "0")
    else:
        monkeypatch.delenv("OCPG_WIN_ATTN_MFMA", raising=False)


def _prepared(case, path, dtype):
    if path == "table":
        return wr.prepared(case, dtype, wr.swin_index(WINDOW)[:case.n, :case.n], wr.table_rows(WINDOW))
    return wr.prepared(case, dtype)


def _on(dev, inp):
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in inp.items()}


def _raw_fwd(d, bias_t, dtype, out, lse):
    from ocpg_amd._lib import check, lib, stream_ptr
    bw, n, _, h, hd = d["qkv"].shape
    check(lib().ocpg_win_attn_fwd(d["qkv"].data_ptr(), bias_t.data_ptr(), d["region"].data_ptr() if d["region"] is not None else None,
                                  d["scale"], bw, d["nw"], n, h, hd, out.data_ptr(), lse.data_ptr(), _DT[dtype], stream_ptr()),
          "ocpg_win_attn_fwd")


@pytest.mark.parametrize("path,dtype", PATHS, ids=PATH_IDS)
@pytest.mark.parametrize("case", wr.CASES, ids=wr.CASE_IDS)
def test_every_path_within_the_derived_bound(dev, monkeypatch, case, path, dtype):
    from ocpg_amd import _lib
    from ocpg_amd.models.ops.functions.win_attn_func import window_attention, window_attention_table
    inp, R, B = _prepared(case, path, dtype)
    d = _on(dev, inp)
    bw, n, h = case.bw, case.n, case.h
    _set_path(monkeypatch, path)
    x = d["qkv"].clone().requires_grad_(True)
    got = {}
    calls = _lib.census(True)
    try:
        if path == "table":
            rows = d["table"].shape[0]
            if _lib.lib().ocpg_win_attn_dtable_supported(n, 32, _DT[dtype], rows) != 1:
                pytest.skip("ocpg_win_attn_dtable_supported(N %d, T %d) == 0: the fused table gradient does not serve this shape" % (n, rows))
            idx2 = _real_index(n).to(dev)
            t = d["table"].clone().requires_grad_(True)
            out = window_attention_table(x, t, idx2, d["region"], d["scale"], d["nw"])
            got["dqkv"], got["dtable"] = torch.autograd.grad(out, (x, t), d["go"])
        else:
            b = d["bias"].clone().requires_grad_(True)
            out = window_attention(x, b, d["region"], d["scale"], d["nw"])
            got["dqkv"], got["dbias"] = torch.autograd.grad(out, (x, b), d["go"])
        calls = dict(calls)
    finally:
        _lib.census(False)
    assert calls.get(_BWD_ENTRY[path], 0) == 1 and not (set(_BWD_ENTRY.values()) - {_BWD_ENTRY[path]}) & set(calls), calls
    assert out.dtype == dtype and got["dqkv"].dtype == dtype
    got["out"] = out
    # lse does not leave the wrapper: the same forward through the raw ABI
    out2, lse = torch.empty_like(out), torch.full((bw, h, n), float("nan"), device=dev)
    _raw_fwd(d, d["bias"].transpose(1, 2).contiguous(), dtype, out2, lse)
    assert torch.equal(out2, out.detach())
    got["lse"] = lse
    res = wr.ratios(got, R, B)
    print("%s %s %s: %s" % (path, dtype, case.name, wr.fmt(res)))
    assert max(res.values()) <= 1.0, res


def _guarded(shape, dtype, dev, zero=False):
    """A contiguous tensor of `shape` inside a larger buffer: GUARD sentinel elements on each side, payload NaN (or zero)."""
    numel = 1
    for s in shape:
        numel *= s
    big = torch.empty(numel + 2 * GUARD, dtype=dtype, device=dev)
    bits = big.view(torch.int32 if dtype == torch.float32 else torch.int16)
    bits.fill_(0x5A5A5A5A if dtype == torch.float32 else 0x5A5A)
    payload = big[GUARD:GUARD + numel].view(shape)
    payload.fill_(0.0 if zero else float("nan"))
    return payload, bits, numel


def _intact(bits, numel):
    sentinel = 0x5A5A5A5A if bits.dtype == torch.int32 else 0x5A5A
    return bool((bits[:GUARD] == sentinel).all()) and bool((bits[GUARD + numel:] == sentinel).all())


@pytest.mark.parametrize("path,dtype", PATHS, ids=PATH_IDS)
@pytest.mark.parametrize("name", ["blocks-n33", "blocks-n65"])
def test_outputs_fully_written_and_nothing_beyond(dev, monkeypatch, name, path, dtype):
    from ocpg_amd._lib import check, lib, stream_ptr
    from ocpg_amd.models.ops.functions.win_attn_func import table_codes
    case = wr.by_name(name)
    inp, R, B = _prepared(case, path, dtype)
    d = _on(dev, inp)
    bw, nw, n, h = case.bw, case.nw, case.n, case.h
    _set_path(monkeypatch, path)
    bias, bias_t = d["bias"].contiguous(), d["bias"].transpose(1, 2).contiguous()
    region = d["region"].data_ptr()
    buf = {"out": _guarded((bw, n, h * 32), dtype, dev), "lse": _guarded((bw, h, n), torch.float32, dev)}
    out, lse = buf["out"][0], buf["lse"][0]
    _raw_fwd(d, bias_t, dtype, out, lse)
    torch.cuda.synchronize()
    for k, (payload, bits, numel) in buf.items():
        assert torch.isfinite(payload).all(), k
        assert _intact(bits, numel), k
    buf = {"dqkv": _guarded(tuple(d["qkv"].shape), dtype, dev), "Dbuf": _guarded((bw, h, n), torch.float32, dev)}
    common = (d["qkv"].data_ptr(), bias.data_ptr(), bias_t.data_ptr(), region, d["scale"], bw, nw, n, h, 32, out.data_ptr(),
              d["go"].data_ptr(), lse.data_ptr(), buf["dqkv"][0].data_ptr(), buf["Dbuf"][0].data_ptr())
    got = {"out": out, "lse": lse, "dqkv": buf["dqkv"][0]}
    if path == "valu":
        buf["dbiasT"] = _guarded((h, n, n), torch.float32, dev, zero=True)
        check(lib().ocpg_win_attn_bwd(*common, buf["dbiasT"][0].data_ptr(), _DT[dtype], stream_ptr()), "ocpg_win_attn_bwd")
        got["dbias"] = buf["dbiasT"][0].transpose(1, 2)
    elif path == "mfma":
        buf["dS"] = _guarded((bw, h, n, n), dtype, dev)
        check(lib().ocpg_win_attn_bwd_mfma(*common, buf["dS"][0].data_ptr(), _DT[dtype], stream_ptr()), "ocpg_win_attn_bwd_mfma")
        got["dbias"] = buf["dS"][0].sum(0, dtype=torch.float32).transpose(1, 2)
    else:
        rows = d["table"].shape[0]
        assert lib().ocpg_win_attn_dtable_supported(n, 32, _DT[dtype], rows) == 1
        code, off = table_codes(_real_index(n).to(dev))
        buf["partials"] = _guarded((bw, h, rows), torch.float32, dev)
        buf["dtable"] = _guarded((rows, h), torch.float32, dev)
        check(lib().ocpg_win_attn_bwd_mfma_dtable(*common, code.data_ptr(), off, rows, buf["partials"][0].data_ptr(),
                                                  buf["dtable"][0].data_ptr(), _DT[dtype], stream_ptr()), "ocpg_win_attn_bwd_mfma_dtable")
        got["dtable"] = buf["dtable"][0]
    torch.cuda.synchronize()
    for k, (payload, bits, numel) in buf.items():
        assert torch.isfinite(payload).all(), k
        assert _intact(bits, numel), k
    # and what was written into the slices is the right answer
    res = wr.ratios(got, R, B)
    print("raw %s %s %s: %s" % (path, dtype, name, wr.fmt(res)))
    assert max(res.values()) <= 1.0, res


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=str)
def test_pretransposed_bias_changes_no_bit(dev, dtype):
    """Two windows: each fp32 dbias element is the sum of two atomic adds onto zero, which no order changes."""
    from ocpg_amd.models.ops.functions.win_attn_func import window_attention
    d = _on(dev, wr.prepared(wr.by_name("blocks-n33"), dtype)[0])
    qkv, go = d["qkv"][:2].contiguous(), d["go"][:2].contiguous()
    res = []
    for bias_t in (None, d["bias"].transpose(1, 2).contiguous(), d["bias"].transpose(1, 2), d["bias"].transpose(1, 2).contiguous().double()):
        x, b = qkv.clone().requires_grad_(True), d["bias"].clone().requires_grad_(True)
        out = window_attention(x, b, d["region"], d["scale"], d["nw"], bias_t)
        res.append((out.detach(),) + torch.autograd.grad(out, (x, b), go))
    for other in res[1:]:          # the pre-transposed table; a view and a wrong dtype, which the wrapper replaces by its own copy
        for got, want in zip(other, res[0]):
            assert torch.equal(got, want)
