"""csrc/roberta.hip on the MI355X: the three kernels against the fp64 references of tests/roberta_ref.py at their derived elementwise
bounds, the whole native encoder against the referee and HF (fp32, CPU), the routing and its fallbacks, and the model end to end."""
import copy

import pytest
import torch

import cases
import roberta_ref as R

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------------------ embed_layer_norm
def _tables(c, v, p, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(v, c, generator=g), torch.randn(p, c, generator=g) * 0.5, torch.randn(c, generator=g) * 0.3,
            1.0 + 0.2 * torch.randn(c, generator=g), torch.randn(c, generator=g) * 0.2)


def _ids(b, l, v, seed, pad=1):
    """pads trailing (row 0 when long enough), interior (every 5th position of row 1) and leading (row 2); ids 0 and V - 1 planted"""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(2, v, (b, l), generator=g)
    ids[0, 0] = 0
    ids[-1, -1] = v - 1
    if l >= 4:
        ids[0, l - l // 4:] = pad
    if b >= 2 and l >= 3:
        ids[1, 2::5] = pad
    if b >= 3:
        ids[2, : l // 3] = pad
    return ids


EMBED_SHAPES = [(1, 1), (2, 5), (3, 64), (2, 65), (2, 130)]


@pytest.mark.parametrize("c", [128, 768])
@pytest.mark.parametrize("b,l", EMBED_SHAPES, ids=[f"{b}x{l}" for b, l in EMBED_SHAPES])
def test_embed_layer_norm_at_the_bound(dev, c, b, l):
    from ocpg_amd.models.ops.functions.roberta_func import embed_layer_norm
    v, p, pad = 50, 140, 1
    word, pos, type0, gamma, beta = _tables(c, v, p, 10 + c + l)
    ids = _ids(b, l, v, 20 + l)
    ref, bound, _ = R.embed_reference(ids, word, pos, type0, gamma, beta, 1e-5, pad)
    got = embed_layer_norm(ids.to(dev), *(t.to(dev) for t in (word, pos, type0, gamma, beta)), 1e-5, pad)
    ratio = R.worst(got, ref, bound)
    print(f"embed_layer_norm C {c} [{b}, {l}]: at {ratio:.3f} of the bound, max |err| {R.max_err(got, ref):.3e}")
    assert ratio <= 1.0


def test_embed_position_table_boundary_and_bad_ids(dev):
    from ocpg_amd._lib import lib, stream_ptr
    from ocpg_amd.models.ops.functions.roberta_func import embed_layer_norm
    c, v, p, pad = 128, 50, 40, 1
    word, pos, type0, gamma, beta = _tables(c, v, p, 31)
    dt = [t.to(dev) for t in (word, pos, type0, gamma, beta)]
    ids = torch.randint(2, v, (2, p - 2), generator=torch.Generator().manual_seed(32))           # no pads: the last token reads row P - 1
    ref, bound, _ = R.embed_reference(ids, word, pos, type0, gamma, beta, 1e-5, pad)
    assert int(R.position_ids(ids, pad).max()) == p - 1
    assert R.worst(embed_layer_norm(ids.to(dev), *dt, 1e-5, pad), ref, bound) <= 1.0
    # one token more: refused by the binding and by the C entry, which launches nothing (the output keeps its fill)
    long_ids = torch.randint(2, v, (1, p - 1), generator=torch.Generator().manual_seed(33)).to(dev)
    with pytest.raises(ValueError, match="position"):
        embed_layer_norm(long_ids, *dt, 1e-5, pad)
    out = torch.full((1, p - 1, c), -7.0, device=dev)
    rc = lib().ocpg_roberta_embed_ln_f32(long_ids.data_ptr(), *(t.data_ptr() for t in dt), 1e-5, pad, 1, p - 1, c, v, p, out.data_ptr(), None,
                                         stream_ptr())
    torch.cuda.synchronize()
    assert rc == -2501 and bool((out == -7.0).all())
    # two ids outside [0, V): counted, their word rows zeros, nothing else disturbed
    ids = _ids(2, 9, v, 34)
    ids[0, 3], ids[1, 8] = v, -5
    ref, bound, nbad = R.embed_reference(ids, word, pos, type0, gamma, beta, 1e-5, pad)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    got = embed_layer_norm(ids.to(dev), *dt, 1e-5, pad, bad=bad)
    assert nbad == 2 and int(bad.item()) == 2 and R.worst(got, ref, bound) <= 1.0
    # C outside the served set
    assert lib().ocpg_roberta_embed_ln_f32(long_ids.data_ptr(), *(t.data_ptr() for t in dt), 1e-5, pad, 1, 4, 126, v, p, out.data_ptr(), None,
                                           stream_ptr()) == -2000


# -------------------------------------------------------------------------------------------------------------------- attention_hd64
def _attend(b, l, seed):
    """row 0: keys in the middle not attended; row 1: exactly one attended key; row 2: all attended"""
    g = torch.Generator().manual_seed(seed)
    att = torch.ones(b, l, dtype=torch.uint8)
    if l >= 3:
        att[0, l // 3: l // 3 + max(1, l // 4)] = 0
    if b >= 2:
        att[1] = 0
        att[1, int(torch.randint(0, l, (1,), generator=g))] = 1
    return att


@pytest.mark.parametrize("b,h", [(1, 1), (3, 2), (1, 12), (3, 12)])
@pytest.mark.parametrize("l", [1, 2, 31, 33, 64, 65, 128])
def test_attention_hd64_at_the_bound(dev, l, b, h):
    from ocpg_amd.models.ops.functions.roberta_func import attention_hd64
    g = torch.Generator().manual_seed(1000 * l + 10 * b + h)
    qkv = torch.randn(b, l, 3, h, 64, generator=g)
    qkv[:, :, 0] *= 1.5
    att = _attend(b, l, l + b)
    ref, bound = R.attention_reference(qkv, att, h, 0.125)
    for mask in (att, att.to(torch.int64)):
        got = attention_hd64(qkv.to(dev).view(b, l, 3 * h * 64), mask.to(dev), h)
        ratio = R.worst(got, ref, bound)
        print(f"attention_hd64 L {l} B {b} H {h} {mask.dtype}: at {ratio:.3f} of the bound, max |err| {R.max_err(got, ref):.3e}")
        assert ratio <= 1.0


def test_attention_hd64_dominant_key_and_limits(dev):
    from ocpg_amd._lib import lib, stream_ptr
    from ocpg_amd.models.ops.functions.roberta_func import attention_hd64
    b, l, h = 2, 70, 2
    g = torch.Generator().manual_seed(77)
    qkv = torch.randn(b, l, 3, h, 64, generator=g)
    qkv[:, :, 1, :, :] *= 0.1
    qkv[:, 66, 1] = 24.0 * qkv[:, 5, 0]                                  # key 66 (second key of lane 2) dominates query 5 by far more than 80
    att = torch.ones(b, l, dtype=torch.uint8)
    ref, bound = R.attention_reference(qkv, att, h, 0.125)
    s = 0.125 * (qkv[:, 5, 0].double() * qkv[:, :, 1].double().permute(1, 0, 2, 3)).sum(-1)          # [L, B, H]
    assert float((s[66] - s[torch.arange(l) != 66].amax(0)).min()) > 80
    got = attention_hd64(qkv.to(dev).view(b, l, -1), att.to(dev), h)
    assert R.worst(got, ref, bound) <= 1.0 and bool(torch.isfinite(got).all())
    out = torch.empty(1, 129, 64, device=dev)
    q129 = torch.zeros(1, 129, 3, 1, 64, device=dev)
    a129 = torch.ones(1, 129, dtype=torch.uint8, device=dev)
    assert lib().ocpg_attn_hd64_fwd_f32(q129.data_ptr(), a129.data_ptr(), 0, 0.125, 1, 129, 1, out.data_ptr(), stream_ptr()) == -2000
    with pytest.raises(ValueError, match="keys"):
        attention_hd64(q129.view(1, 129, -1), a129, 1)


# -------------------------------------------------------------------------------------------------------------------------- bias_act
@pytest.mark.parametrize("act", ["none", "gelu", "tanh"])
@pytest.mark.parametrize("r,c", [(7, 132), (7, 131), (64, 3072)])
def test_bias_act_at_the_bound(dev, act, r, c):
    from ocpg_amd.models.ops.functions.roberta_func import bias_act
    g = torch.Generator().manual_seed(r * c)
    x = torch.randn(r, c, generator=g) * 2
    special = torch.tensor([0.0, 1e-8, 1.0, 6.0, 30.0])
    x[0, :10] = torch.cat([special, -special])
    bias = torch.randn(c, generator=g) * 0.5
    bias[:10] = 0.0                                                     # the planted values reach the activation as they are
    for bb in (bias, None):
        ref, bound = R.bias_act_reference(x, bb, act)
        xd = x.to(dev)
        got = bias_act(xd, None if bb is None else bb.to(dev), act)
        ratio = R.worst(got, ref, bound)
        print(f"bias_act {act} [{r}, {c}] bias {bb is not None}: at {ratio:.3f} of the bound, max |err| {R.max_err(got, ref):.3e}")
        assert ratio <= 1.0 and torch.equal(xd.cpu(), x)
        alias = bias_act(xd, None if bb is None else bb.to(dev), act, out=xd)
        assert alias.data_ptr() == xd.data_ptr() and torch.equal(alias, got)


# --------------------------------------------------------------------------------------------------------------------- whole encoder
@pytest.fixture(scope="module")
def models():
    return {"tiny": R.seeded_model(R.tiny_config(), seed=0), "base2": R.seeded_model(R.base2_config(), seed=1)}


@pytest.mark.parametrize("l", [5, 40])
@pytest.mark.parametrize("name", ["tiny", "base2"])
def test_native_encoder_against_referee_and_hf(dev, models, monkeypatch, name, l):
    from ocpg_amd import _lib
    from ocpg_amd.models import fallbacks
    from ocpg_amd.models.text_encoder import roberta_native
    cpu = models[name]
    # the 40-row position table of the tiny configuration holds 38 tokens (positions 2 .. 39): L = 40 runs as 38 there
    ids, att = R.padded_ids(2, min(l, cpu.config.max_position_embeddings - 2), cpu.config.vocab_size, seed=40 + l)
    hf_h, hf_p = R.hf_forward(cpu, ids, att)
    ref_h, ref_p = R.referee_of(cpu, ids, att)
    gpu = copy.deepcopy(cpu).to(dev)
    monkeypatch.setenv("OCPG_STRICT_HIP", "1")
    fallbacks.reset()
    calls = _lib.census(True)
    try:
        with torch.no_grad():                                            # as TextEncoder.forward calls a frozen encoder
            got_h, got_p = roberta_native.encode(gpu, ids, att)
        torch.cuda.synchronize()
    finally:
        _lib.census(False)
    assert fallbacks.snapshot() == {}
    layers = cpu.config.num_hidden_layers
    assert calls.get("ocpg_roberta_embed_ln_f32") == 1 and calls.get("ocpg_attn_hd64_fwd_f32") == layers
    assert calls.get("ocpg_bias_act_f32") == layers + 1 and calls.get("ocpg_dropout_add_ln_fwd") == 2 * layers
    for what, got, hf, ref in (("hidden", got_h, hf_h, ref_h), ("pooler", got_p, hf_p, ref_p)):
        own, theirs = R.max_err(got, ref), R.max_err(hf, ref)
        print(f"{name} L {ids.shape[1]} {what}: native {own:.3e}  HF fp32 on the CPU {theirs:.3e}")
        assert own <= 4 * theirs, (what, own, theirs)


def test_training_mode_dropout_keeps_hf(dev, models, monkeypatch):
    from ocpg_amd.models import fallbacks
    monkeypatch.delenv("OCPG_STRICT_HIP", raising=False)
    from ocpg_amd.models.text_encoder import roberta_native
    gpu = copy.deepcopy(models["tiny"]).to(dev).train()
    for p in gpu.parameters():
        p.requires_grad_(False)
    ids, att = R.padded_ids(2, 6, 100, seed=50)
    fallbacks.reset()
    with pytest.warns(RuntimeWarning, match="training-mode dropout"), torch.no_grad():
        h, p = roberta_native.encode(gpu, ids, att)
    assert sum(fallbacks.snapshot().values()) == 1 and h.shape == (2, 6, 128) and p.shape == (2, 128)
    fallbacks.reset()


# ------------------------------------------------------------------------------------------------------------------------ end to end
def _model(golden, dev):
    """The infer_collate configuration at 256 channels (every attention on the HIP kernels) with a 2-layer RoBERTa of RoBERTa-base's
    width behind the hash tokenizer, eval mode."""
    from ocpg_amd.models import build_model
    from ocpg_amd.models.text_encoder.text_encoder import HashTokenizer
    g = golden("infer_collate")
    torch.manual_seed(0)
    model, _, _ = build_model(cases.default_args(device=str(dev), **dict(g.meta["cfg"], hidden_dim=256, mask_dim=256, dim_feedforward=256)))
    backbone = R.seeded_model(R.base2_config(), seed=3)
    for p in backbone.parameters():
        p.requires_grad_(False)
    model.text_encoder.tokenizer = HashTokenizer(backbone.config.vocab_size)
    model.text_encoder.text_backbone = backbone
    return model.to(dev).eval(), g


def test_model_forward_switch_on_against_off(golden, dev):
    model, g = _model(golden, dev)
    frames = g["infer_frames"][:2].to(dev)
    targets = [{"size": torch.as_tensor([int(frames.shape[-2]), int(frames.shape[-1])], device=dev)}]
    caption = ["the person on the left riding a red bike"]
    out = {}
    with torch.no_grad():
        for native in (False, True):
            model.text_encoder.native = native
            out[native] = model([frames], caption, targets)["pred_masks"].float().cpu()
    err = (out[True] - out[False]).abs()
    print(f"pred_masks, switch on vs off: max |diff| {err.max().item():.3e} (max |ref| {out[False].abs().max().item():.3f})")
    assert bool((err <= 1e-3 + 2e-5 * out[False].abs()).all()) and out[False].std().item() > 1e-3


@pytest.mark.parametrize("native_text", [False, True], ids=["hf", "native-text"])
def test_segment_video_encodes_once_and_keeps_the_masks(golden, dev, native_text):
    from ocpg_amd import inference
    from ocpg_amd.models.ops.functions.mask_tail_func import mask_probabilities
    import model_checks
    model, g = _model(golden, dev)
    model_checks.to_channels_last(model)
    model.text_encoder.native = native_text
    frames = g["infer_frames"].to(dev)                                   # 5 frames: clips of 2 + 2 + 1
    caption, clip, amp = "a small dog near the tree", 2, torch.bfloat16
    size = torch.as_tensor([int(frames.shape[-2]), int(frames.shape[-1])], device=dev)
    logits, low = [], []
    with torch.no_grad():
        for start in range(0, frames.shape[0], clip):                    # the loop as it was: the string to every clip
            with torch.autocast("cuda", dtype=amp):
                o = model.forward_selected([frames[start:start + clip]], [caption], [{"size": size}])
            logits.append(o["pred_logits"][0, :, 0])
            low.append(o["pred_masks_low"][0].float())
        want = mask_probabilities(torch.cat(low, 0), o["mask_up"], tuple(frames.shape[-2:]), tuple(frames.shape[-2:]))
    got_logits, got = inference.segment_video(model, frames, caption, clip_len=clip, amp_dtype=amp, native=True)
    assert torch.equal(got_logits, torch.cat(logits, 0)) and torch.equal(got, want)
    assert got.std().item() > 1e-4
