"""csrc/attn_smallk.hip and csrc/attn_longk.hip against the fp64 reference of tests/attn_ref.py, each output element held to the bound
derived there: |got - ref| <= bound, no multiplier, no max|ref|, no other kernel as the yardstick (tests/test_attn_bounds_cpu.py shows
what this harness sees and what the older criterion does not).

(a) out, lse, dq, dk, dv of every case in fp32 / bf16 / fp16 through `attention()` and autograd, q a strided view of a packed [Lq, B, 2C]
    tensor whose other half gets an exactly zero gradient; the census proves which entry point served the call; the same forward through
    the raw ABI gives lse and a bit-equal out.  The cases: one key, one head, the backward's key bounds 8 / 9 and 16 / 17, peaked
    softmaxes, the short-key forward at 28 / 29 / 32 keys and 8 heads (dynamic LDS below and above 64 KiB), gpb = 2 on either kernel
    with a last workgroup that holds one ragged token group, every window layout of the long-key backward, a planted padded key.
(b) The batch-first form (one launch per entry, k / v row stride B C) under the same bound.
(c) 1, 9 and 32 keys through ocpg_attn_longk_fwd / _bwd, which serve them as a one-chunk window, under the long-key bound.
(d) Through the raw ABI with every output a slice of a larger buffer, out / dq with row stride 2C: payloads pre-filled with NaN (dk / dv
    with zeros) come back finite, the guard bands and the gaps between rows keep their sentinel bits.
(e) dk / dv rows of a padded key are exactly zero.
(f) Dropout: the keep mask is recovered once from the kernel in fp32 (q = k = 0, one-hot values) and fed to the reference for all three
    dtypes.
(g) The 8-head, 32-key forward launches with its 73 856 B of dynamic LDS: `attention()` returns a tensor under OCPG_STRICT_HIP=1.

The worst measured ratios are in DESIGN.md section 4.8b.
"""
import pytest
import torch

import attn_ref as ar

pytestmark = pytest.mark.gpu

_DT = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
GUARD = 4096
RNG = (20240607, 11)
PLAIN = [c for c in ar.CASES if c.pdrop == 0]
DROPOUT = [c for c in ar.CASES if c.pdrop > 0]
_ENTRY = {"short": ("ocpg_attn_smallk_fwd", "ocpg_attn_smallk_bwd"), "long": ("ocpg_attn_longk_fwd", "ocpg_attn_longk_bwd")}
_KEEP = {}


def _names(cases):
    return [c.name for c in cases]


def _route(monkeypatch, kernel):
    """`attention()` serves more than MAX_KEYS keys on the long-key kernels only when forced."""
    if kernel == "long":
        monkeypatch.setenv("OCPG_ATTN_LONGK", "force")
    else:
        monkeypatch.delenv("OCPG_ATTN_LONGK", raising=False)


def _pad_ptr(d):
    pad = None if d["key_pad"] is None else d["key_pad"].to(torch.uint8).contiguous()
    return pad, (None if pad is None else pad.data_ptr())


def _raw_fwd(kernel, d, q, ldq, out, ldo, lse, pdrop=0.0, rng=(0, 0)):
    from ocpg_amd._lib import check, lib, stream_ptr
    lq, b, c = d["q"].shape
    h, lk = d["h"], d["k"].shape[0]
    pad, pp = _pad_ptr(d)
    fn = getattr(lib(), _ENTRY[kernel][0])
    check(fn(q.data_ptr(), ldq, d["k"].data_ptr(), c, d["v"].data_ptr(), c, pp, d["scale"], lq, b, h, 32, lk, pdrop, rng[0], rng[1], None,
             out.data_ptr(), ldo, lse.data_ptr(), _DT[d["q"].dtype], stream_ptr()), _ENTRY[kernel][0])


def _raw_bwd(kernel, d, q, ldq, out, ldo, lse, dq, lddq, dk, dv, pdrop=0.0, rng=(0, 0)):
    from ocpg_amd._lib import check, lib, stream_ptr
    lq, b, c = d["q"].shape
    h, lk = d["h"], d["k"].shape[0]
    pad, pp = _pad_ptr(d)
    fn = getattr(lib(), _ENTRY[kernel][1])
    head = (q.data_ptr(), ldq, d["k"].data_ptr(), c, d["v"].data_ptr(), c, pp, d["go"].data_ptr(), c)
    saved = (lse.data_ptr(),) if kernel == "short" else (out.data_ptr(), ldo, lse.data_ptr())
    check(fn(*head, *saved, d["scale"], lq, b, h, 32, lk, pdrop, rng[0], rng[1], None, dq.data_ptr(), lddq, dk.data_ptr(), dv.data_ptr(),
             _DT[d["q"].dtype], stream_ptr()), _ENTRY[kernel][1])


def _report(tag, got, R, B, terms=None):
    """Worst ratios, printed; for an output over its bound also the element, what came back, the reference, the bound there and
    (`terms`: a function that returns the bound's labelled summands) the term that dominates it."""
    res = ar.ratios(got, R, B)
    print("%s: %s" % (tag, ar.fmt(res)))
    for name, worst in res.items():
        if not worst <= 1.0:
            x = got[name].detach().double()
            r = ((x - R[name]).abs() / B[name]).nan_to_num(float("inf")).flatten()
            i = int(r.argmax())
            idx = tuple(int(j) for j in torch.unravel_index(torch.tensor(i), x.shape))
            print("  %s over its bound at %s: got %.9g ref %.9g bound %.3g ratio %.3g; largest term of the bound: %s" %
                  (name, idx, x.flatten()[i].item(), R[name].flatten()[i].item(), B[name].flatten()[i].item(), r[i].item(),
                   ar.dominant(terms(), name, i) if terms else "?"))
    return res


def _through_attention(dev, monkeypatch, case, dtype, keep=None):
    """(a) / (f): attention() + autograd on a strided q, then the raw forward for lse."""
    from ocpg_amd import _lib
    from ocpg_amd.models.ops.functions import attn_smallk_func as f
    inp, R, B = ar.prepared(case, dtype, dev, keep=keep)
    d = inp
    lq, b, c = d["q"].shape
    h = d["h"]
    _route(monkeypatch, case.kernel)
    rng = RNG if case.pdrop > 0 else None
    qk = torch.cat([d["q"], d["go"]], -1).requires_grad_(True)             # packed [Lq, B, 2C]: q is the first half
    ki, vi = (t.clone().requires_grad_(True) for t in (d["k"], d["v"]))
    calls = _lib.census(True)
    try:
        out = f.attention(qk[..., :c], ki, vi, d["key_pad"], d["scale"], h, case.pdrop, rng)
        assert out is not None, "attention() declined the shape"
        gq, gk, gv = torch.autograd.grad(out, (qk, ki, vi), d["go"])
        calls = dict(calls)
    finally:
        _lib.census(False)
    fwd, bwd = _ENTRY[case.kernel]
    other = set(_ENTRY["long" if case.kernel == "short" else "short"])
    assert calls.get(fwd, 0) == 1 and calls.get(bwd, 0) == 1 and not other & set(calls), calls
    assert out.dtype == dtype and gq.dtype == dtype and gk.dtype == dtype and gv.dtype == dtype
    assert gq[..., c:].abs().max().item() == 0                              # the other half of the packed projection gets no gradient
    out2 = torch.full((lq, b, c), float("nan"), dtype=dtype, device=dev)
    lse = torch.full((lq, b, h), float("nan"), dtype=torch.float32, device=dev)
    _raw_fwd(case.kernel, d, qk.detach(), 2 * c, out2, c, lse, case.pdrop, RNG if case.pdrop > 0 else (0, 0))
    assert torch.equal(out2, out.detach())
    res = _report("attention %s %s" % (case.name, dtype), dict(out=out, lse=lse, dq=gq[..., :c], dk=gk, dv=gv), R, B,
                  lambda: ar.bounds(R, dtype, case.kernel, ar.case_geometry(case), terms=True)[1])
    assert max(res.values()) <= 1.0, res


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("case", PLAIN, ids=_names(PLAIN))
def test_every_output_within_the_derived_bound(dev, monkeypatch, case, dtype):
    _through_attention(dev, monkeypatch, case, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("case", [c for c in PLAIN if c.b <= 3], ids=_names([c for c in PLAIN if c.b <= 3]))
def test_batch_first_within_the_derived_bound(dev, monkeypatch, case, dtype):
    from ocpg_amd import _lib
    from ocpg_amd.models.ops.functions import attn_smallk_func as f
    d, R, B = ar.prepared(case, dtype, dev)
    geo = ar.geometry(case.kernel, case.lq, 1, case.h, case.lk)             # one launch per batch entry
    if geo["chain"] != ar.case_geometry(case)["chain"]:
        B = ar.bounds(R, dtype, case.kernel, geo)
    _route(monkeypatch, case.kernel)
    qb = d["q"].transpose(0, 1).contiguous().requires_grad_(True)
    ki, vi = (t.clone().requires_grad_(True) for t in (d["k"], d["v"]))
    calls = _lib.census(True)
    try:
        out = f.attention_batch_first(qb, ki, vi, d["key_pad"], d["scale"], d["h"])
        assert out is not None, "attention_batch_first() declined the shape"
        gq, gk, gv = torch.autograd.grad(out, (qb, ki, vi), d["go"].transpose(0, 1).contiguous())
        calls = dict(calls)
    finally:
        _lib.census(False)
    fwd, bwd = _ENTRY[case.kernel]
    other = set(_ENTRY["long" if case.kernel == "short" else "short"])
    assert calls.get(fwd, 0) == case.b and calls.get(bwd, 0) == case.b and not other & set(calls), calls
    res = _report("batch-first %s %s" % (case.name, dtype), dict(out=out.transpose(0, 1), dq=gq.transpose(0, 1), dk=gk, dv=gv), R, B,
                  lambda: ar.bounds(R, dtype, case.kernel, geo, terms=True)[1])
    assert max(res.values()) <= 1.0, res


def _raw_all(kernel, d, dev):
    """Forward and backward through the raw ABI on plain contiguous buffers: out, lse, dq (NaN-filled), dk, dv (fp32, zero-filled)."""
    lq, b, c = d["q"].shape
    lk, dtype = d["k"].shape[0], d["q"].dtype
    out = torch.full((lq, b, c), float("nan"), dtype=dtype, device=dev)
    lse = torch.full((lq, b, d["h"]), float("nan"), dtype=torch.float32, device=dev)
    dq = torch.full((lq, b, c), float("nan"), dtype=dtype, device=dev)
    dkv = torch.zeros(2, lk, b, c, dtype=torch.float32, device=dev)
    _raw_fwd(kernel, d, d["q"], c, out, c, lse)
    _raw_bwd(kernel, d, d["q"], c, out, c, lse, dq, c, dkv[0], dkv[1])
    return dict(out=out, lse=lse, dq=dq, dk=dkv[0], dv=dkv[1])


SHORT_ON_LONG = [c for c in PLAIN if c.kernel == "short" and c.lk in (1, 9, 32)]


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("case", SHORT_ON_LONG, ids=_names(SHORT_ON_LONG))
def test_short_keys_through_the_long_key_entry_points(dev, case, dtype):
    """check_dims of csrc/attn_longk.hip admits 1-128 keys; 32 or fewer dispatch the one-chunk window at key 0.  That entry ships."""
    d, R, B = ar.prepared(case, dtype, dev, kernel="long", abi=True)          # dk / dv in fp32: no rounding term of the wrapper's
    res = _report("long-key ABI %s %s" % (case.name, dtype), _raw_all("long", d, dev), R, B,
                  lambda: ar.bounds(R, dtype, "long", ar.case_geometry(case, "long"), terms=True, abi=True)[1])
    assert max(res.values()) <= 1.0, res


def _guarded(shape, dtype, dev, ld=None, zero=False):
    """A [..., c] tensor with row stride `ld` inside a larger buffer: GUARD sentinel elements on each side and ld - c between the rows,
    payload NaN (or zero).  Returns the payload view and a function that tells whether every sentinel bit is unchanged."""
    lead, c = tuple(shape[:-1]), shape[-1]
    ld = ld or c
    rows = 1
    for s in lead:
        rows *= s
    numel = rows * ld
    big = torch.empty(numel + 2 * GUARD, dtype=dtype, device=dev)
    sentinel = 0x5A5A5A5A if dtype == torch.float32 else 0x5A5A
    bits = big.view(torch.int32 if dtype == torch.float32 else torch.int16)
    bits.fill_(sentinel)
    payload = big[GUARD:GUARD + numel].view(*lead, ld)[..., :c]
    payload.fill_(0.0 if zero else float("nan"))

    def intact():
        body = bits[GUARD:GUARD + numel].view(rows, ld)
        return bool((bits[:GUARD] == sentinel).all()) and bool((bits[GUARD + numel:] == sentinel).all()) and bool((body[:, c:] == sentinel).all())
    return payload, intact


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("name", ["s-k9", "l-k65-peaked"])
def test_outputs_fully_written_and_nothing_beyond(dev, name, dtype):
    case = ar.by_name(name)
    d, R, B = ar.prepared(case, dtype, dev, abi=True)                         # dk / dv in fp32: no rounding term of the wrapper's
    lq, b, c = d["q"].shape
    lk, h = case.lk, case.h
    buf = {"out": _guarded((lq, b, c), dtype, dev, ld=2 * c), "lse": _guarded((lq, b, h), torch.float32, dev),
           "dq": _guarded((lq, b, c), dtype, dev, ld=2 * c), "dk": _guarded((lk, b, c), torch.float32, dev, zero=True),
           "dv": _guarded((lk, b, c), torch.float32, dev, zero=True)}
    got = {k: v[0] for k, v in buf.items()}
    _raw_fwd(case.kernel, d, d["q"], c, got["out"], 2 * c, got["lse"])
    _raw_bwd(case.kernel, d, d["q"], c, got["out"], 2 * c, got["lse"], got["dq"], 2 * c, got["dk"], got["dv"])
    torch.cuda.synchronize()
    for k, (payload, intact) in buf.items():
        assert torch.isfinite(payload).all(), k
        assert intact(), k
    # and what was written into the slices is the right answer
    res = _report("guarded %s %s" % (name, dtype), got, R, B,
                  lambda: ar.bounds(R, dtype, case.kernel, ar.case_geometry(case), terms=True, abi=True)[1])
    assert max(res.values()) <= 1.0, res


PADDED = [c for c in PLAIN if c.pad != "none"]


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("case", PADDED, ids=_names(PADDED))
def test_padded_keys_get_no_gradient(dev, case, dtype):
    d = ar.prepared(case, dtype, dev)[0]
    got = _raw_all(case.kernel, d, dev)
    pad = d["key_pad"].transpose(0, 1)                                       # [Lk, B]
    assert int(pad.sum()) > 0
    assert bool((got["dk"][pad] == 0).all()) and bool((got["dv"][pad] == 0).all())
    assert bool((got["dk"][~pad] != 0).any()) and bool((got["dv"][~pad] != 0).any())


def _recovered_keep(dev, monkeypatch, case):
    """keep [B, H, Lq, Lk] (0 or 1/(1-p)) of RNG, from the kernel itself in fp32: with q = k = 0 every weight is 1 / Lk, and with the
    unit vector d as the value of key 32 c + d, channel d of the output is the dropped weight of that key (chunk c)."""
    if case.name not in _KEEP:
        from ocpg_amd.models.ops.functions import attn_smallk_func as f
        _route(monkeypatch, case.kernel)
        lq, b, h, lk = case.lq, case.b, case.h, case.lk
        c = h * 32
        zq, zk = torch.zeros(lq, b, c, device=dev), torch.zeros(lk, b, c, device=dev)
        parts = []
        for c0 in range(0, lk, 32):
            n = min(32, lk - c0)
            onehot = torch.zeros(lk, b, h, 32, device=dev)
            for j in range(n):
                onehot[c0 + j, :, :, j] = 1.0
            parts.append(f.attention(zq, zk, onehot.view(lk, b, c), None, ar.SCALE, h, case.pdrop, RNG).view(lq, b, h, 32)[..., :n])
        w = torch.cat(parts, -1)                                             # [Lq, B, H, Lk]
        keep = torch.where(w != 0, torch.full_like(w, ar.keep_value(case.pdrop)), torch.zeros_like(w))
        assert torch.allclose(w, keep / lk, rtol=1e-6, atol=0)
        assert 0.6 < (keep > 0).float().mean().item() < 0.8
        _KEEP[case.name] = keep.permute(1, 2, 0, 3).contiguous()
    return _KEEP[case.name]


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("case", DROPOUT, ids=_names(DROPOUT))
def test_dropout_within_the_derived_bound(dev, monkeypatch, case, dtype):
    _through_attention(dev, monkeypatch, case, dtype, keep=_recovered_keep(dev, monkeypatch, case))


def test_eight_heads_32_keys_forward_launches(dev, monkeypatch):
    """2304 Lk + 128 bytes of dynamic LDS at 8 heads: 73 856 B at 32 keys, past the default 64-KiB window.  The launch must be served:
    attention() returns a tensor under OCPG_STRICT_HIP=1 and nothing is counted as a fallback."""
    from ocpg_amd import _lib
    from ocpg_amd.models import fallbacks
    from ocpg_amd.models.ops.functions import attn_smallk_func as f
    case = ar.by_name("s-k32")
    assert (2 * case.lk * case.h * 36 + 32) * 4 == 73856
    d = ar.prepared(case, torch.bfloat16, dev)[0]
    monkeypatch.delenv("OCPG_ATTN_LONGK", raising=False)
    monkeypatch.setenv("OCPG_STRICT_HIP", "1")
    fallbacks.reset()
    calls = _lib.census(True)
    try:
        out = f.attention(d["q"], d["k"], d["v"], d["key_pad"], d["scale"], d["h"])
        calls = dict(calls)
    finally:
        _lib.census(False)
    torch.cuda.synchronize()
    assert torch.is_tensor(out) and out.shape == d["q"].shape and bool(torch.isfinite(out).all())
    assert calls == {"ocpg_attn_smallk_fwd": 1}, calls
    assert fallbacks.snapshot() == {}
