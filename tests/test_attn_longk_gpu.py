"""csrc/attn_longk.hip: multi-head attention against 33 .. 128 keys (long captions in the text gate, more than 32 decoder queries),
the kernels alone against fp64, their dropout stream, graph replays, and the routing of the modules that use them."""
import ctypes
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu

SCALE = 32 ** -0.5


def _mha_core_reference(q, k, v, pad, scale, H, keep=None):
    """softmax(q k^T * scale + key padding) [* keep] v in plain tensor ops on [L, B, C] inputs, in fp64."""
    Lq, B, C = q.shape
    hd = C // H
    qh, kh, vh = (t.double().reshape(t.shape[0], B, H, hd).permute(1, 2, 0, 3) for t in (q, k, v))      # [B,H,L,hd]
    s = torch.matmul(qh, kh.transpose(-1, -2)) * scale
    if pad is not None:
        s = s.masked_fill(pad[:, None, None, :], float("-inf"))
    p = s.softmax(-1)
    if keep is not None:
        p = p * keep.double()
    return torch.matmul(p, vh).permute(2, 0, 1, 3).reshape(Lq, B, C)


def _padding(Lq, B, H, Lk, dev):
    """The key padding of each kernel case; every batch element keeps an unpadded key (a fully padded row is NaN in the reference too)."""
    if (Lq, B, H, Lk) in ((5, 10, 8, 50), (19, 1, 1, 96)):
        return None
    pad = torch.zeros(B, Lk, dtype=torch.bool, device=dev)
    if Lk == 33:
        pad[0, Lk - 2:] = True                       # the one key past the first chunk is padded
    elif Lk == 64:
        pad[0, :32] = True                           # a whole FIRST chunk masked: m stays -inf across the chunk boundary
        pad[1, 0] = True
        pad[1, 32:] = True                           # a whole LAST chunk masked
    elif Lk == 45:
        pad[0, Lk - 2:] = True
        pad[1, 0] = True
        pad[2, 28:37] = True                         # a run across the chunk boundary
    else:                                            # 128
        pad[0, Lk - 2:] = True
        pad[1, 0] = True
        pad[1, 60:70] = True
    assert not pad.all(1).any()
    return pad


# fp32: the short-key kernel's own bound; 16-bit storage: one rounding of the result (2^-9 / 2^-11 relative) is far inside 2e-2
_TOL = {torch.float32: 2e-5, torch.bfloat16: 2e-2, torch.float16: 2e-2}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("Lq,B,H,Lk", [(77, 1, 4, 33), (300, 2, 2, 64), (1237, 3, 8, 45), (5, 10, 8, 50), (70, 2, 8, 128), (19, 1, 1, 96)])
def test_long_key_attention_kernel(dev, dtype, Lq, B, H, Lk, monkeypatch):
    """out, dq, dk, dv of csrc/attn_longk.hip against the tensor-op formulation in fp64 on the same (rounded) operands: one key past a
    chunk, whole chunks masked, a token count below one token group, the maximum key count, one head; q is a strided view.
    (OCPG_ATTN_LONGK=force: every key count the kernels serve, also past the measured default bound MAX_KEYS.)"""
    from ocpg_amd import _lib
    from ocpg_amd.models.ops.functions import attn_smallk_func as f
    monkeypatch.setenv("OCPG_ATTN_LONGK", "force")
    C = H * 32
    g = torch.Generator(device="cpu").manual_seed(Lq + Lk)
    qk = torch.randn(Lq, B, 2 * C, generator=g).to(dev).to(dtype)
    q = qk[..., :C]                                                       # strided view (row stride 2C)
    k = (torch.randn(Lk, B, C, generator=g) * 1.5).to(dev).to(dtype)
    v = torch.randn(Lk, B, C, generator=g).to(dev).to(dtype)
    go = torch.randn(Lq, B, C, generator=g).to(dev).to(dtype)
    pad = _padding(Lq, B, H, Lk, dev)
    qi, ki, vi = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    ref = _mha_core_reference(qi, ki, vi, pad, SCALE, H)
    want = [ref.detach()] + list(torch.autograd.grad((ref * go.double()).sum(), (qi, ki, vi)))
    qi = qk.detach().clone().requires_grad_(True)
    ki, vi = (t.detach().clone().requires_grad_(True) for t in (k, v))
    calls = _lib.census(True)
    try:
        out = f.attention(qi[..., :C], ki, vi, pad, SCALE, H)
        assert out is not None, "attention() declined a long-key shape"
        got = [out.detach()] + list(torch.autograd.grad((out.float() * go.float()).sum(), (qi, ki, vi)))
    finally:
        _lib.census(False)
    assert calls.get("ocpg_attn_longk_fwd", 0) == 1 and calls.get("ocpg_attn_longk_bwd", 0) == 1, calls
    assert got[1][..., C:].abs().max().item() == 0                        # the other half of the packed projection gets no gradient
    got[1] = got[1][..., :C]
    tol = _TOL[dtype]
    errs = []
    for a, r, name in zip(got, want, ("out", "dq", "dk", "dv")):
        errs.append((name, (a.double() - r).abs().max().item(), r.abs().max().item()))
    print(dtype, (Lq, B, H, Lk), errs)
    for name, err, mx in errs:
        assert err <= tol * mx + 1e-6, (name, err, mx)

    # every element of out / lse / dq is written: the same calls through the C ABI on NaN-filled buffers (dk / dv are accumulated into)
    dt = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}[dtype]
    nan = float("nan")
    o2 = torch.full((Lq, B, C), nan, dtype=dtype, device=dev)
    lse = torch.full((Lq, B, H), nan, dtype=torch.float32, device=dev)
    dq2 = torch.full((Lq, B, C), nan, dtype=dtype, device=dev)
    dkv = torch.zeros(2, Lk, B, C, dtype=torch.float32, device=dev)
    p8 = None if pad is None else pad.to(torch.uint8).contiguous()
    pp = None if p8 is None else p8.data_ptr()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    L = _lib.lib()
    assert L.ocpg_attn_longk_fwd(q.data_ptr(), 2 * C, k.data_ptr(), C, v.data_ptr(), C, pp, SCALE, Lq, B, H, 32, Lk, 0.0, 0, 0, None,
                                 o2.data_ptr(), C, lse.data_ptr(), dt, st) == 0
    assert L.ocpg_attn_longk_bwd(q.data_ptr(), 2 * C, k.data_ptr(), C, v.data_ptr(), C, pp, go.data_ptr(), C, o2.data_ptr(), C, lse.data_ptr(),
                                 SCALE, Lq, B, H, 32, Lk, 0.0, 0, 0, None, dq2.data_ptr(), C, dkv[0].data_ptr(), dkv[1].data_ptr(), dt, st) == 0
    assert torch.isfinite(lse).all()
    assert torch.equal(o2, got[0]) and torch.equal(dq2, got[1])
    for a, r, name in zip((dkv[0], dkv[1]), want[2:], ("dk", "dv")):
        assert (a.double() - r).abs().max().item() <= tol * r.abs().max().item() + 1e-6, name


def _weights(f, q, k, Lk, H, p, rng):
    """The (dropped) attention weights [Lq, B, H, Lk], recovered chunk by chunk with one-hot values: for chunk c the value of key
    32 c + d is the unit vector d of every head, so channel d of the output IS the weight of that key."""
    Lq, B, C = q.shape
    parts = []
    for c0 in range(0, Lk, 32):
        n = min(32, Lk - c0)
        onehot = torch.zeros(Lk, B, H, 32, device=q.device)
        for d in range(n):
            onehot[c0 + d, :, :, d] = 1.0
        parts.append(f.attention(q, k, onehot.view(Lk, B, C), None, SCALE, H, p, rng).view(Lq, B, H, 32)[..., :n])
    return torch.cat(parts, -1)


def test_long_key_attention_dropout(dev, monkeypatch):
    """Attention-weight dropout over three chunks: the mask is a pure function of (seed, offset) with an index that does not collide
    past key 32, keeps ~1-p of the weights scaled by 1/(1-p), and the backward draws the SAME mask."""
    from ocpg_amd.models.ops.functions import attn_smallk_func as f
    monkeypatch.setenv("OCPG_ATTN_LONGK", "force")
    Lq, B, H, Lk, p = 640, 3, 8, 70, 0.3
    C = H * 32
    g = torch.Generator(device="cpu").manual_seed(3)
    q, k = torch.randn(Lq, B, C, generator=g).to(dev), torch.randn(Lk, B, C, generator=g).to(dev)
    rng = (20240607, 11)
    probs = _weights(f, q, k, Lk, H, p, rng)
    clean = _weights(f, q, k, Lk, H, 0.0, None)
    keep = torch.where(probs != 0, torch.full_like(probs, 1 / (1 - p)), torch.zeros_like(probs))
    assert torch.allclose(probs, clean * keep, rtol=1e-5, atol=1e-7)
    rate = (keep > 0).float().mean().item()
    print("keep rate", rate)
    assert abs(rate - (1 - p)) < 0.02
    # no two key columns share their decisions (the short-key index row * 32 + j would repeat column j at j + 32 of the next row)
    kept = (keep > 0).flatten(0, 2).float()
    agree = (kept[1:, :32] == kept[:-1, 32:64]).float().mean().item()
    assert abs(agree - (p * p + (1 - p) ** 2)) < 0.02, agree
    assert torch.equal(probs, _weights(f, q, k, Lk, H, p, rng))
    assert not torch.equal(probs, _weights(f, q, k, Lk, H, p, (rng[0], rng[1] + 1)))
    v = torch.randn(Lk, B, C, generator=g).to(dev)
    go = torch.randn(Lq, B, C, generator=g).to(dev)
    qi, ki, vi = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    out = f.attention(qi, ki, vi, None, SCALE, H, p, rng)
    got = [out.detach()] + list(torch.autograd.grad((out * go).sum(), (qi, ki, vi)))
    qi, ki, vi = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    ref = _mha_core_reference(qi, ki, vi, None, SCALE, H, keep.permute(1, 2, 0, 3))
    want = [ref.detach()] + list(torch.autograd.grad((ref * go.double()).sum(), (qi, ki, vi)))
    for a, r, name in zip(got, want, ("out", "dq", "dk", "dv")):
        err, mx = (a.double() - r).abs().max().item(), r.abs().max().item()
        print(name, err, mx)
        assert err <= 2e-5 * mx + 1e-6, (name, err, mx)


def test_long_key_dropout_masks_advance_under_replay(dev):
    """A captured forward + backward with dropout draws a new mask on every replay (the offset base lives in device memory), and
    replay r equals eager call r from the same host counter: bit for bit, except dk / dv, whose fp32 atomics arrive in any order."""
    from ocpg_amd.models.ops.functions import attn_smallk_func as af
    from ocpg_amd.models.ops.functions import fused_ln_func as f
    torch.manual_seed(78)
    Lq, B, H, Lk, p = 40, 2, 2, 40, 0.25
    q = torch.randn(Lq, B, H * 32, device=dev, requires_grad=True)
    k = torch.randn(Lk, B, H * 32, device=dev, requires_grad=True)
    v = torch.randn(Lk, B, H * 32, device=dev, requires_grad=True)
    go = torch.randn(Lq, B, H * 32, device=dev)

    def step():
        o = af.attention(q, k, v, None, SCALE, H, p)
        return [t.detach().clone() for t in (o,) + torch.autograd.grad((o * go).sum(), (q, k, v))]

    saved = f.get_rng_state()
    try:
        f.set_rng_state({"dropout_calls": 500})
        eager = [step() for _ in range(3)]
        assert f.get_rng_state()["dropout_calls"] == 503
        assert not torch.equal(eager[0][0], eager[1][0])
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            step()                      # warm the side stream before the capture
        torch.cuda.synchronize()
        f.set_rng_state({"dropout_calls": 500})
        rng = f.GraphRng(dev)
        graph = torch.cuda.CUDAGraph()
        with rng, torch.cuda.graph(graph, stream=side):
            static = step()
            rng.advance()
        rng.finalize()
        assert rng.calls == 1 and f.get_rng_state()["dropout_calls"] == 500        # a capture runs nothing
        for r in range(3):
            graph.replay()
            rng.replayed()
            torch.cuda.synchronize()
            for i, (got, want) in enumerate(zip(static, eager[r])):
                if i < 2:
                    assert torch.equal(got, want), (r, i, (got - want).abs().max().item())
                else:
                    assert (got - want).abs().max().item() <= 1e-6 * want.abs().max().item(), (r, i)
        assert f.get_rng_state()["dropout_calls"] == 503
    finally:
        f.set_rng_state(saved)


def _grads(out, go, inputs, module):
    module.zero_grad()
    (out * go).sum().backward()
    return [out.detach()] + [t.grad.clone() for t in inputs] + [p.grad.clone() for p in module.parameters()]


def _close(got, want):
    for i, (a, r) in enumerate(zip(got, want)):
        assert torch.allclose(a, r, rtol=2e-4, atol=2e-5), (i, (a - r).abs().max().item(), r.abs().max().item())


def test_modules_route_long_keys_to_the_hip_kernels(dev, monkeypatch):
    """MultiheadAttention (query is key, 40 queries: the many-query decoder case) and the text gate (40 text keys, padded; both layouts)
    at d_model 64 / 2 heads run csrc/attn_longk.hip under OCPG_STRICT_HIP=1 with no counted fallback, and agree with the same module
    objects on the library path (attention.HIP_SMALLK off: what served these key counts before)."""
    from ocpg_amd import _lib
    from ocpg_amd.models import attention, fallbacks
    from ocpg_amd.models.segmentation import VisionLanguageFusionModule
    monkeypatch.delenv("OCPG_STRICT_HIP", raising=False)
    torch.manual_seed(5)
    c, H, lk, b = 64, 2, 40, 3
    mha = attention.MultiheadAttention(c, H).to(dev)
    fuse = VisionLanguageFusionModule(c, H).to(dev)
    x = torch.randn(lk, b, c, device=dev)
    val = torch.randn(lk, b, c, device=dev)
    gx = torch.randn(lk, b, c, device=dev)
    t, h, w = 2, 5, 7
    vis = torch.randn(b, t * h * w, c, device=dev)                       # batch-first; the token-major form is a view of it
    text = torch.randn(lk, b, c, device=dev)
    pos = torch.randn(lk, b, c, device=dev)
    pad = torch.zeros(b, lk, dtype=torch.bool, device=dev)
    pad[0, 30:], pad[2, 35:], pad[1, 0] = True, True, True
    gv = torch.randn(b, t * h * w, c, device=dev)

    def run(batch_first):
        xi, vi = x.clone().requires_grad_(True), val.clone().requires_grad_(True)
        a = _grads(mha(xi, xi, vi), gx, (xi, vi), mha)
        v_, tx = vis.clone().requires_grad_(True), text.clone().requires_grad_(True)
        if batch_first:
            o = fuse.forward_batch_first(v_, tx, pad, pos)
            assert o is not None
        else:
            tok = v_.view(b, t, h, w, c).permute(1, 2, 3, 0, 4)
            o = fuse(visual=tok, text=tx, text_key_padding_mask=pad, text_pos=pos).view(t * h * w, b, c).transpose(0, 1)
        return a, _grads(o, gv, (v_, tx), fuse)

    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        monkeypatch.setattr(attention, "HIP_SMALLK", False)
        want_mha, want_fuse = run(False)
        monkeypatch.setattr(attention, "HIP_SMALLK", True)
    monkeypatch.delenv("OCPG_ATTN_LONGK", raising=False)
    monkeypatch.setenv("OCPG_STRICT_HIP", "1")
    fallbacks.reset()
    for batch_first in (False, True):
        calls = _lib.census(True)
        try:
            got_mha, got_fuse = run(batch_first)
        finally:
            _lib.census(False)
        n = 1 + (b if batch_first else 1)
        assert calls.get("ocpg_attn_longk_fwd", 0) == n and calls.get("ocpg_attn_longk_bwd", 0) == n, calls
        assert "ocpg_attn_smallk_fwd" not in calls and "ocpg_attn_smallk_bwd" not in calls, calls
        _close(got_mha, want_mha)
        _close(got_fuse, want_fuse)
    assert fallbacks.snapshot() == {}
    monkeypatch.delenv("OCPG_STRICT_HIP")

    # past what the kernels serve the module still answers, through the counted library path
    big = torch.randn(129, b, c, device=dev)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        calls = _lib.census(True)
        try:
            o = mha(big, big, big)
        finally:
            _lib.census(False)
        monkeypatch.setattr(attention, "HIP_SMALLK", False)
        ref = mha(big, big, big)
    assert not any(s.startswith("ocpg_attn_") for s in calls), calls
    assert any(key.startswith("MultiheadAttention") for key in fallbacks.snapshot())
    assert torch.allclose(o, ref, rtol=2e-4, atol=2e-5)
    fallbacks.reset()


def test_short_keys_and_the_switch_keep_the_earlier_paths(dev, monkeypatch):
    """Up to 32 keys still run csrc/attn_smallk.hip, and OCPG_ATTN_LONGK=0 hands more than 32 keys back to the caller's library path."""
    from ocpg_amd import _lib
    from ocpg_amd.models.ops.functions import attn_smallk_func as f
    H, C = 2, 64
    q = torch.randn(50, 2, C, device=dev, requires_grad=True)
    calls = _lib.census(True)
    try:
        for lk in (20, 32):
            k, v = torch.randn(lk, 2, C, device=dev), torch.randn(lk, 2, C, device=dev)
            f.attention(q, k, v, None, SCALE, H).sum().backward()
            assert f.attention_batch_first(q.detach().transpose(0, 1), k, v, None, SCALE, H) is not None
    finally:
        _lib.census(False)
    assert calls.get("ocpg_attn_smallk_fwd", 0) == 2 + 2 * 2 and calls.get("ocpg_attn_smallk_bwd", 0) == 2, calls
    assert not any("longk" in s for s in calls), calls
    k, v = torch.randn(40, 2, C, device=dev), torch.randn(40, 2, C, device=dev)
    monkeypatch.setenv("OCPG_ATTN_LONGK", "0")
    assert f.attention(q, k, v, None, SCALE, H) is None
    assert f.attention_batch_first(q.detach().transpose(0, 1), k, v, None, SCALE, H) is None
    monkeypatch.delenv("OCPG_ATTN_LONGK")
    assert f.attention(q, k, v, None, SCALE, H) is not None
    # the default bound is the measured one; =force serves whatever the kernels can
    k, v = torch.randn(128, 2, C, device=dev), torch.randn(128, 2, C, device=dev)
    assert (f.attention(q, k, v, None, SCALE, H) is None) == (f.MAX_KEYS < 128)
    monkeypatch.setenv("OCPG_ATTN_LONGK", "force")
    assert f.attention(q, k, v, None, SCALE, H) is not None
    assert f.attention(q, torch.randn(129, 2, C, device=dev), torch.randn(129, 2, C, device=dev), None, SCALE, H) is None
