"""csrc/text_gate.hip (the fusion gate with its projections folded into the text side) against the plain formula in fp64.

Reference: query projection -> per-head softmax attention over the text keys with the padding mask -> out_proj -> multiply, in fp64 on
the module's own parameters, autograd supplying the reference gradients.  Compared: out, dx and the gradients of in_proj_weight,
in_proj_bias, out_proj.weight, out_proj.bias and of the text.

Bound: the softmax amplifies score error by the spread of the data, so no closed form; the UNFUSED module path (the code the fused gate
replaces: cast, q GEMM, attn_smallk, out_proj GEMM, multiply) runs on the same inputs in the same test and the fused path's max
elementwise error against fp64 must be at most 2x the unfused path's, for every compared tensor (both make a handful of 16-bit roundings
and differ only in which; an indexing or layout bug shows at 10x or more).  Both errors are printed; DESIGN.md section 4.8o records them.

Shapes: B = 2, L in {1, 70, 193} (one token, ragged last tiles, several workgroups), Lk in {1, 6, 9, 16} (every padded row count the
kernels are built for: 32 / 64 / 96 / 128 rows), L = 700 at 9 keys (more than one token range in the parameter kernel) and L = 19 200 at 9 keys (the benchmark's finest level: a
workgroup walks several rounds of token tiles, 32 token ranges); clip 0 has its
last two keys padded (from 3 keys on), clip 1 none; bf16 and fp16.  x is scaled so that the scores spread over a few units.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

C, H, B = 256, 8, 2
SHAPES = [(L, Lk) for L in (1, 70, 193) for Lk in (1, 6, 9, 16)] + [(700, 9), (19200, 9)]
NAMES = ("out", "dx", "in_proj_weight", "in_proj_bias", "out_proj.weight", "out_proj.bias", "text")
_CACHE = {}


def _module():
    from ocpg_amd.models.segmentation import VisionLanguageFusionModule
    if "mod" not in _CACHE:
        torch.manual_seed(1234)
        mod = VisionLanguageFusionModule(C, H).cuda()
        with torch.no_grad():
            mod.multihead_attn.in_proj_bias.normal_(0, 0.2)
            mod.multihead_attn.out_proj.bias.normal_(0, 0.2)
        _CACHE["mod"] = mod
    return _CACHE["mod"]


def _data(L, Lk):
    key = ("data", L, Lk)
    if key not in _CACHE:
        gen = torch.Generator(device="cuda").manual_seed(1000 * L + Lk)
        d = {"x": 4.0 * torch.randn(B, L, C, device="cuda", generator=gen),
             "text": torch.randn(Lk, B, C, device="cuda", generator=gen),
             "pos": 0.5 * torch.randn(Lk, B, C, device="cuda", generator=gen),
             "g": torch.randn(B, L, C, device="cuda", generator=gen),
             "pad": torch.zeros(B, Lk, dtype=torch.bool, device="cuda")}
        if Lk >= 3:
            d["pad"][0, -2:] = True
        _CACHE[key] = d
    return _CACHE[key]


def _reference(L, Lk):
    """The plain formula in fp64: {name: tensor}; computed once per shape and never modified."""
    key = ("ref", L, Lk)
    if key not in _CACHE:
        d, a = _data(L, Lk), _module().multihead_attn
        x = d["x"].double().requires_grad_()
        text = d["text"].double().requires_grad_()
        w = a.in_proj_weight.detach().double().requires_grad_()
        b = a.in_proj_bias.detach().double().requires_grad_()
        wo = a.out_proj.weight.detach().double().requires_grad_()
        bo = a.out_proj.bias.detach().double().requires_grad_()
        wq, wk, wv = w.chunk(3)
        bq, bk, bv = b.chunk(3)
        q = (x @ wq.t() + bq).view(B, L, H, 32)
        k = ((text + d["pos"].double()) @ wk.t() + bk).view(Lk, B, H, 32)
        v = (text @ wv.t() + bv).view(Lk, B, H, 32)
        s = torch.einsum("blhd,kbhd->bhlk", q, k) * 32 ** -0.5
        p = s.masked_fill(d["pad"][:, None, None, :], float("-inf")).softmax(-1)
        o = torch.einsum("bhlk,kbhd->blhd", p, v).reshape(B, L, C)
        out = x * (o @ wo.t() + bo)
        grads = torch.autograd.grad(out, (x, w, b, wo, bo, text), d["g"].double())
        _CACHE[key] = dict(zip(NAMES, (out.detach(),) + grads))
    return _CACHE[key]


def _run(monkeypatch, fused, dtype, d, kernel_forward=False):
    """The module's gate on batch-first tokens (forward_tokens) under autocast, forward and backward -> ({name: tensor}, census of library calls)."""
    from ocpg_amd import _lib
    from ocpg_amd.models.ops.functions import text_gate_func
    monkeypatch.setattr(text_gate_func, "ENABLED", fused)
    monkeypatch.setattr(text_gate_func, "FUSED_FORWARD", kernel_forward)
    mod = _module()
    mod.zero_grad(set_to_none=True)
    x, text = d["x"].clone().requires_grad_(), d["text"].clone().requires_grad_()
    _lib.census(True)
    try:
        with torch.autocast("cuda", dtype=dtype):
            out = mod.forward_tokens(x, text, d["pad"], d["pos"])
        assert out is not None and out.dtype == torch.float32
        out.backward(d["g"])
        torch.cuda.synchronize()
    finally:
        calls = dict(_lib.census(False))
    a = mod.multihead_attn
    got = (out.detach(), x.grad, a.in_proj_weight.grad, a.in_proj_bias.grad, a.out_proj.weight.grad, a.out_proj.bias.grad, text.grad)
    return {n: t.detach().clone() for n, t in zip(NAMES, got)}, calls


@pytest.mark.parametrize("mode", ["bwd", "fwd"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("L,Lk", SHAPES)
def test_fused_gate_against_fp64(monkeypatch, L, Lk, dtype, mode):
    """mode bwd (the default): the forward is the unfused path's, bit for bit, the backward the kernels'; fwd (OCPG_TEXT_GATE_FUSED=fwd):
    the forward through the kernel too."""
    d, ref = _data(L, Lk), _reference(L, Lk)
    fused, calls_f = _run(monkeypatch, True, dtype, d, mode == "fwd")
    plain, calls_p = _run(monkeypatch, False, dtype, d)
    assert calls_f.get("ocpg_text_gate_bwd_h16") == 1 and "ocpg_attn_smallk_bwd" not in calls_f, calls_f
    if mode == "fwd":
        assert calls_f.get("ocpg_text_gate_fwd_h16") == 1 and "ocpg_attn_smallk_fwd" not in calls_f, calls_f
    else:
        assert calls_f.get("ocpg_attn_smallk_fwd") == B and "ocpg_text_gate_fwd_h16" not in calls_f, calls_f
        assert torch.equal(fused["out"], plain["out"])
    assert not any(k.startswith("ocpg_text_gate_") for k in calls_p), calls_p
    assert calls_p.get("ocpg_attn_smallk_fwd") == B and calls_p.get("ocpg_attn_smallk_bwd") == B, calls_p
    worst = []
    for n in NAMES:
        assert torch.isfinite(fused[n]).all(), n
        ef = (fused[n].double() - ref[n]).abs().max().item()
        ep = (plain[n].double() - ref[n]).abs().max().item()
        print(f"text_gate {mode} L={L} Lk={Lk} {dtype}: {n:16s} fused err {ef:.4e}  unfused err {ep:.4e}  ratio {ef / max(ep, 1e-300):.3f}"
              f"  max|ref| {ref[n].abs().max().item():.3e}")
        if not ef <= 2.0 * ep:
            worst.append((n, ef, ep))
    assert not worst, f"fused error above 2x the unfused path's: {worst}"


def test_padded_keys_get_no_gradient_through_the_gate(monkeypatch):
    """Clip 0's two padded keys: their value rows cannot reach the output, so the text gradient there comes from the key side only and is
    zero too (a padded key's score is masked)."""
    d = _data(70, 9)
    fused, _ = _run(monkeypatch, True, torch.bfloat16, d)
    assert fused["text"][-2:, 0].abs().max().item() == 0.0
    assert fused["text"][-2:, 1].abs().max().item() > 0.0


def test_more_than_16_keys_declined(monkeypatch):
    """Lk = 17: -2000 from both entry points with nothing written, and the module still gives the unfused result."""
    from ocpg_amd._lib import lib, stream_ptr
    L, Lk = 70, 17
    gen = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn(B, L, C, device="cuda", generator=gen)
    kp = torch.randn(B, H * Lk, C, device="cuda", generator=gen).bfloat16()
    c = torch.randn(B, H * Lk, device="cuda", generator=gen)
    bo = torch.randn(C, device="cuda", generator=gen)
    out = torch.full_like(x, 7.0)
    part = torch.full((1, B, 2 * 144 * C + 144 + C), 7.0, device="cuda")
    ws = torch.full((2, B, L, 144), 7.0, device="cuda", dtype=torch.bfloat16)
    assert lib().ocpg_text_gate_rows(Lk) == 0
    rc = lib().ocpg_text_gate_fwd_h16(x.data_ptr(), kp.data_ptr(), kp.data_ptr(), c.data_ptr(), bo.data_ptr(), None, 0.17, B, L, C, H, Lk,
                                      out.data_ptr(), 1, stream_ptr())
    assert rc == -2000
    rc = lib().ocpg_text_gate_bwd_h16(x.data_ptr(), x.data_ptr(), kp.data_ptr(), kp.data_ptr(), c.data_ptr(), bo.data_ptr(), None, 0.17, B, L, C,
                                      H, Lk, out.data_ptr(), part.data_ptr(), ws.data_ptr(), 1, stream_ptr())
    assert rc == -2000
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (part == 7.0).all() and (ws == 7.0).all()
    # other refusals: another width / head count, a misaligned pointer
    assert lib().ocpg_text_gate_fwd_h16(x.data_ptr(), kp.data_ptr(), kp.data_ptr(), c.data_ptr(), bo.data_ptr(), None, 0.17, B, L, 128, H, 9,
                                        out.data_ptr(), 1, stream_ptr()) == -2000
    assert lib().ocpg_text_gate_fwd_h16(x.data_ptr() + 4, kp.data_ptr(), kp.data_ptr(), c.data_ptr(), bo.data_ptr(), None, 0.17, B, L - 1, C, H, 9,
                                        out.data_ptr(), 1, stream_ptr()) == -2000
    assert (out == 7.0).all()

    d = {"x": x, "text": torch.randn(Lk, B, C, device="cuda", generator=gen), "pos": torch.randn(Lk, B, C, device="cuda", generator=gen),
         "g": torch.randn(B, L, C, device="cuda", generator=gen), "pad": torch.zeros(B, Lk, dtype=torch.bool, device="cuda")}
    on, calls_on = _run(monkeypatch, True, torch.bfloat16, d)
    off, calls_off = _run(monkeypatch, False, torch.bfloat16, d)
    assert calls_on == calls_off and not any(k.startswith("ocpg_text_gate_") for k in calls_on), (calls_on, calls_off)
    for n in NAMES:
        assert torch.equal(on[n], off[n]), n


def test_fp32_is_not_routed(monkeypatch):
    """Without autocast the module keeps its calls (fp32 is out of the kernels' scope)."""
    from ocpg_amd import _lib
    d = _data(70, 9)
    _lib.census(True)
    try:
        out = _module().forward_tokens(d["x"], d["text"], d["pad"], d["pos"])
        torch.cuda.synchronize()
    finally:
        calls = dict(_lib.census(False))
    assert out is not None and not any(k.startswith("ocpg_text_gate_") for k in calls), calls


def test_inference_keeps_the_unfused_calls(monkeypatch):
    """torch.no_grad() under autocast (evaluation): the gate declines, the census is the unfused path's with none of the new symbols, and
    the output is bit for bit what the switch at 0 gives."""
    from ocpg_amd import _lib
    from ocpg_amd.models.ops.functions import text_gate_func
    d, res = _data(70, 9), []
    for on in (True, False):
        monkeypatch.setattr(text_gate_func, "ENABLED", on)
        _lib.census(True)
        try:
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                assert not _module().fused_gate_serves(d["x"], d["text"])
                out = _module().forward_tokens(d["x"], d["text"], d["pad"], d["pos"])
            torch.cuda.synchronize()
        finally:
            res.append((out, dict(_lib.census(False))))
    assert res[0][1] == res[1][1] and res[0][1].get("ocpg_attn_smallk_fwd") == B, res[0][1]
    assert not any(k.startswith("ocpg_text_gate_") for k in res[0][1]), res[0][1]
    assert torch.equal(res[0][0], res[1][0])


def test_unfused_path_that_declines_is_not_an_error(monkeypatch):
    """The unfused forward returns None (its attention kernel does not serve the call): forward_tokens returns what forward_batch_first
    does, None, and launches nothing of its own."""
    from ocpg_amd import _lib
    from ocpg_amd.models import attention
    from ocpg_amd.models.ops.functions import text_gate_func
    monkeypatch.setattr(text_gate_func, "ENABLED", True)
    monkeypatch.setattr(text_gate_func, "FUSED_FORWARD", False)
    monkeypatch.setattr(attention, "HIP_SMALLK", False)
    d = _data(70, 9)
    _lib.census(True)
    try:
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = _module().forward_tokens(d["x"].clone().requires_grad_(), d["text"], d["pad"], d["pos"])
    finally:
        calls = dict(_lib.census(False))
    assert out is None and not any(k.startswith("ocpg_text_gate_") for k in calls), calls


def _level(monkeypatch, fused, src, text, d, shared):
    """OCPG._fuse_level (the model's route to the gate) on a stand-in model whose LFM blocks are the identity."""
    import types

    from ocpg_amd.models import ocpg
    from ocpg_amd.models.ops.functions import text_gate_func
    monkeypatch.setattr(text_gate_func, "ENABLED", fused)
    monkeypatch.setattr(text_gate_func, "FUSED_FORWARD", False)
    m = types.SimpleNamespace(input_fft=[lambda s, hf: (s, hf)], input_fft_post=[lambda s, hf: (s, hf)], fusion_module=_module())
    m._gate_token_major = lambda *a: ocpg.OCPG._gate_token_major(m, *a)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        return ocpg.OCPG._fuse_level(m, 0, src, B, 2, text, d["pad"], d["pos"], None, shared)[0]


def test_model_route_keeps_the_forward_and_shares_the_operands(monkeypatch):
    """_fuse_level on two channels-last maps [(b t), 256, h, w] of one forward: the outputs are bit for bit the switch-off (token-major)
    ones, the census shows the token-major forward launches and one fused backward per level, the text-side operands are built once for
    both levels (the forward's `shared` dict).  The gradients are checked for the ROUTE only (the map's layout in and out of the
    backward): what test_fused_gate_against_fp64 holds to fp64 are the same kernels, and both paths sit about 1e-2 of the largest entry
    from fp64 there, so 5e-2 of the largest entry separates roundings from a permuted or transposed gradient (order 1)."""
    from ocpg_amd import _lib
    from ocpg_amd.models.ops.functions import text_gate_func
    mod, d = _module(), _data(70, 9)
    gen = torch.Generator(device="cuda").manual_seed(77)
    maps = [torch.randn(B * 2, C, h, w, device="cuda", generator=gen).contiguous(memory_format=torch.channels_last) for h, w in ((5, 7), (3, 4))]
    gos = [torch.randn(B * 2, C, h, w, device="cuda", generator=gen) for h, w in ((5, 7), (3, 4))]
    built, real, res = [], text_gate_func.text_operands, []
    monkeypatch.setattr(text_gate_func, "text_operands", lambda *a: built.append(1) or real(*a))
    for fused in (True, False):
        mod.zero_grad(set_to_none=True)
        srcs, text = [m.clone().requires_grad_() for m in maps], d["text"].clone().requires_grad_()
        shared = {}
        _lib.census(True)
        try:
            outs = [_level(monkeypatch, fused, s_, text, d, shared) for s_ in srcs]
            sum((o * g).sum() for o, g in zip(outs, gos)).backward()
            torch.cuda.synchronize()
        finally:
            calls = dict(_lib.census(False))
        res.append([o.detach() for o in outs] + [s_.grad for s_ in srcs] + [text.grad] + [p.grad.clone() for p in mod.multihead_attn.parameters()])
        if fused:
            assert len(built) == 1 and "text_gate" in shared
            assert calls.get("ocpg_attn_smallk_fwd") == 2 and calls.get("ocpg_text_gate_bwd_h16") == 2, calls
            assert "ocpg_attn_smallk_bwd" not in calls and "ocpg_text_gate_fwd_h16" not in calls, calls
        else:
            assert len(built) == 1 and not any(k.startswith("ocpg_text_gate_") for k in calls), calls
    for i, (a, r) in enumerate(zip(*res)):
        if i < 2:
            assert torch.equal(a, r), i
        else:
            assert (a - r).abs().max().item() <= 5e-2 * r.abs().max().item(), (i, (a - r).abs().max().item(), r.abs().max().item())


def test_two_forwards_on_the_same_text_tensors(monkeypatch):
    """Nothing of a forward is kept after it: the same text tensor gated and back-propagated twice (no parameter update between) works and
    gives the same gradients."""
    from ocpg_amd.models.ops.functions import text_gate_func
    monkeypatch.setattr(text_gate_func, "ENABLED", True)
    monkeypatch.setattr(text_gate_func, "FUSED_FORWARD", False)
    mod, d, got = _module(), _data(70, 9), []
    text = d["text"].clone().requires_grad_()
    for _ in range(2):
        mod.zero_grad(set_to_none=True)
        text.grad = None
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = mod.forward_tokens(d["x"].clone().requires_grad_(), text, d["pad"], d["pos"])
        out.backward(d["g"])
        got.append([text.grad.clone()] + [p.grad.clone() for p in mod.multihead_attn.parameters()])
    for a, b in zip(*got):
        assert torch.equal(a, b)
