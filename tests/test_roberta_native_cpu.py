"""The native RoBERTa text encoder without a GPU: the fp64 referee (tests/roberta_ref.py) against HF, the runner on the CPU compositions of
its kernels against the referee, position ids and key masks, the limits, the stacked-weight cache, and the routing through TextEncoder and
the inference clip loop."""
import copy

import pytest
import torch

import roberta_ref as R

REFEREE_VS_HF = 5e-6        # hidden 128, 2 layers: 8 x the 6.2e-7 measured for HF fp32 against the referee (slack for another BLAS)


@pytest.fixture(scope="module")
def tiny():
    return R.seeded_model(R.tiny_config(), seed=0)


def _args(**over):
    from ocpg_amd.opts import default_args
    return default_args(**over)


def _follows_hf(model, ids, att):
    """roberta_forward on `model` within 4 x HF's own error of the referee, hidden states and pooler; -> the hidden states"""
    from ocpg_amd.models.text_encoder.roberta_native import roberta_forward
    hf_h, hf_p = R.hf_forward(model, ids, att)
    ref_h, ref_p = R.referee_of(model, ids, att)
    got_h, got_p = roberta_forward(model, ids, att)
    assert got_h.dtype == torch.float32 and got_h.shape == ref_h.shape and got_p.shape == ref_p.shape
    for name, got, hf, ref in (("hidden", got_h, hf_h, ref_h), ("pooler", got_p, hf_p, ref_p)):
        own, theirs = R.max_err(got, ref), R.max_err(hf, ref)
        print(f"{tuple(ids.shape)} {name}: runner {own:.3e}  HF {theirs:.3e}")
        assert own <= 4 * theirs, (name, own, theirs)
    return got_h


def test_referee_agrees_with_hf(tiny):
    ids, att = R.padded_ids(3, 12, 100, seed=1)
    hf_h, hf_p = R.hf_forward(tiny, ids, att)
    ref_h, ref_p = R.referee_of(tiny, ids, att)
    eh, ep = R.max_err(hf_h, ref_h), R.max_err(hf_p, ref_p)
    print(f"HF fp32 vs fp64 referee: hidden {eh:.3e} pooler {ep:.3e}")
    assert bool(att[1:].eq(0).any())                                    # pad rows are compared too
    assert eh <= REFEREE_VS_HF and ep <= REFEREE_VS_HF


@pytest.mark.parametrize("l", [5, 38])
def test_runner_on_cpu_compositions_against_referee(tiny, l):
    ids, att = R.padded_ids(2, l, 100, seed=2)
    _follows_hf(tiny, ids, att)


def test_position_ids_and_masks(tiny):
    from ocpg_amd.models.ops.functions.roberta_func import position_ids
    ids = torch.tensor([[0, 5, 1, 7, 2, 1], [0, 9, 2, 1, 1, 1]])
    want = torch.tensor([[2, 3, 1, 4, 5, 1], [2, 3, 4, 1, 1, 1]])
    assert torch.equal(position_ids(ids, 1), want) and torch.equal(R.position_ids(ids, 1), want)
    outs = []
    for att in (torch.tensor([[1, 1, 1, 0, 1, 0], [1, 1, 1, 0, 0, 0]]), ids.ne(1).long()):
        outs.append(_follows_hf(tiny, ids, att))
    assert (outs[0] - outs[1]).abs().max().item() > 1e-3               # the mask, not the ids, decides which keys are read


def test_limits(tiny):
    from ocpg_amd.models.text_encoder.roberta_native import roberta_forward
    ids = torch.randint(3, 100, (1, 38), generator=torch.Generator().manual_seed(3))          # P = 40: positions 2 .. 39
    assert int(R.position_ids(ids, 1).max()) == 39
    _follows_hf(tiny, ids, torch.ones_like(ids))
    ids39 = torch.randint(3, 100, (1, 39), generator=torch.Generator().manual_seed(4))
    with pytest.raises(ValueError, match="position"):
        roberta_forward(tiny, ids39, torch.ones_like(ids39))
    bad = ids.clone()
    bad[0, 7] = 100
    with pytest.raises(ValueError, match="token id"):
        roberta_forward(tiny, bad, torch.ones_like(bad))
    ids2, att2 = R.padded_ids(2, 6, 100, seed=5)
    att2[1] = 0
    with pytest.raises(ValueError, match="attends no key"):
        roberta_forward(tiny, ids2, att2)


def test_ops_are_forward_only():
    from ocpg_amd.models.ops.functions import roberta_func as rf
    x = torch.randn(3, 8, requires_grad=True)
    with pytest.raises(RuntimeError, match="forward only"):
        rf.bias_act(x, None, "gelu")
    with pytest.raises(RuntimeError, match="forward only"):
        rf.attention_hd64(torch.randn(1, 2, 3 * 64, requires_grad=True), torch.ones(1, 2, dtype=torch.uint8), 1)
    w = torch.randn(10, 8, requires_grad=True)
    with pytest.raises(RuntimeError, match="forward only"):
        rf.embed_layer_norm(torch.zeros(1, 2, dtype=torch.long), w, torch.randn(6, 8), torch.randn(8), torch.ones(8), torch.zeros(8), 1e-5, 1)


def test_weight_cache_follows_the_module(tiny):
    from ocpg_amd.models.text_encoder.roberta_native import roberta_forward
    model = copy.deepcopy(tiny)
    ids, att = R.padded_ids(2, 7, 100, seed=6)
    first, _ = roberta_forward(model, ids, att)
    other = R.seeded_model(R.tiny_config(), seed=11)
    model.load_state_dict(other.state_dict())
    got = _follows_hf(model, ids, att)
    want, _ = R.referee_of(other, ids, att)
    assert R.max_err(got, want) <= 4 * R.max_err(R.hf_forward(other, ids, att)[0], want) and (got - first).abs().max().item() > 1e-2
    with torch.no_grad():
        model.encoder.layer[1].attention.self.key.weight.mul_(3.0)
    got2 = _follows_hf(model, ids, att)
    assert (got2 - got).abs().max().item() > 1e-4


def _text_encoder(native, backbone):
    from ocpg_amd.models.text_encoder.text_encoder import HashTokenizer, TextEncoder
    enc = TextEncoder(_args(text_encoder_lazy=True, text_encoder_native=native))
    enc.tokenizer = HashTokenizer(backbone.config.vocab_size)
    enc.text_backbone = copy.deepcopy(backbone)
    return enc


def test_switch_reading_and_state_dict_keys(tiny, monkeypatch):
    monkeypatch.delenv("OCPG_TEXT_NATIVE", raising=False)
    off, on = _text_encoder(None, tiny), _text_encoder(True, tiny)
    assert off.native is False and on.native is True
    monkeypatch.setenv("OCPG_TEXT_NATIVE", "1")
    assert _text_encoder(None, tiny).native is True and _text_encoder(False, tiny).native is False
    on(["a small dog", "the person on the left"], torch.device("cpu"))
    from ocpg_amd.models.text_encoder.roberta_native import roberta_forward
    ids, att = R.padded_ids(1, 4, 100, seed=7)
    roberta_forward(on.text_backbone, ids, att)                          # builds the stacked-weight cache on the owned module
    assert list(on.state_dict().keys()) == list(off.state_dict().keys())
    assert [n for n, _ in on.named_parameters()] == [n for n, _ in off.named_parameters()]
    assert [n for n, _ in on.named_buffers()] == [n for n, _ in off.named_buffers()]


def test_cpu_text_encoder_keeps_hf_with_the_switch_on(tiny):
    from ocpg_amd.models import fallbacks
    from ocpg_amd.models.text_encoder.text_encoder import PrecomputedText
    texts = ["a small dog", "the person on the left riding a red bike"]
    off, on = _text_encoder(False, tiny), _text_encoder(True, tiny)
    fallbacks.reset()
    a, b = off(texts, torch.device("cpu")), on(texts, torch.device("cpu"))
    assert fallbacks.snapshot() == {}                                    # CPU tensors: the host-logic case, not a counted fallback
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and b[2].dtype == torch.bool and bool(b[2][0].any())
    for enc in (off, on):
        pre = enc.precompute(texts, torch.device("cpu"))
        assert isinstance(pre, PrecomputedText) and all(torch.equal(x, y) for x, y in zip(pre, a))
        assert not pre.features.requires_grad
        assert all(torch.equal(x, y) for x, y in zip(enc(pre, torch.device("cpu")), a))


def test_clip_loop_encodes_an_expression_once():
    from ocpg_amd import inference
    from ocpg_amd.models.text_encoder.text_encoder import PrecomputedText
    calls = {"encode": 0, "clips": []}

    class Encoder:
        text_backbone = object()

        def precompute(self, texts, device):
            calls["encode"] += 1
            assert texts == ["a zebra"]
            return PrecomputedText(torch.zeros(1, 3, 768), torch.zeros(1, 768), torch.zeros(1, 3, dtype=torch.bool))

    class Stub(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.text_encoder = Encoder()

        def forward_selected(self, clips, captions, targets):
            calls["clips"].append(captions)
            t, _, h, w = clips[0].shape
            return {"pred_logits": torch.zeros(1, t, 1, 1), "pred_masks_low": torch.zeros(1, t, h // 4, w // 4), "mask_up": 4}

    logits, masks = inference.segment_video(Stub(), torch.zeros(6, 3, 16, 16), "a zebra", clip_len=2, native=True)
    assert calls["encode"] == 1 and len(calls["clips"]) == 3 and all(isinstance(c, PrecomputedText) for c in calls["clips"])
    assert all(c is calls["clips"][0] for c in calls["clips"]) and masks.shape == (6, 16, 16)
