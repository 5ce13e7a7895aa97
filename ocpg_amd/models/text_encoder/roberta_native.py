"""The frozen RoBERTa text encoder on the project's own kernels (opt-in).

`roberta_forward(text_backbone, input_ids, attention_mask)` runs the forward of the HF `RobertaModel` that TextEncoder owns, reading
THAT module's parameters: nothing is copied into a second module, so state-dict keys, optimizer groups and checkpoints are what they
were.  fp32 and forward only, with autocast disabled whatever the caller's autocast state (under 16-bit autocast HF would run its
Linears in 16 bit: this path's features are closer to fp32 than the default path's).

Arithmetic (what tests/roberta_ref.py restates in fp64):

    position ids   pad + #{j <= l : ids[b, j] != pad} where ids[b, l] != pad, else pad      (from the IDS, not from attention_mask)
    x = LN(word[ids] + pos[position ids] + type[0])
    per layer:     a = attention(x Wqkv^T + bqkv), scale 1/sqrt(64), keys with attention_mask == 0 at probability exactly 0
                   x = LN(a Wo^T + bo + x)
                   h = gelu_erf(x W1^T + b1)
                   x = LN(h W2^T + b2 + x)
    pooler = tanh(x[:, 0] Wp^T + bp)
    LN eps from the config; no dropout anywhere (eval mode, or both probabilities 0).

Launches per call on a GPU: 1 (embeddings + LN) + 8 per layer (qkv product, attention, output product, add + LN, product, bias + GELU,
product, add + LN) + 2 (pooler product, bias + tanh) = 99 for RoBERTa-base.

The stacked [3C, C] q / k / v weight and [3C] bias are built once per layer and kept on the HF module's layer object; they are rebuilt
when any of the six source tensors changed (`_version` or `data_ptr()`): load_state_dict and in-place updates are seen.
"""
import torch

from .. import fallbacks
from ..ops.functions import roberta_func as rf

_CACHE_ATTR = "_ocpg_qkv_cache"


def why_not(text_backbone, input_ids):
    """None when the native path serves this call, else the reason (one short phrase) why HF keeps it."""
    cfg = text_backbone.config
    p = text_backbone.embeddings.word_embeddings.weight
    if not p.is_cuda:
        return "parameters not on a GPU"
    params = list(text_backbone.parameters())
    if any(q.dtype != torch.float32 for q in params):
        return "parameters not fp32"
    c, h = cfg.hidden_size, cfg.num_attention_heads
    if c != h * rf.HEAD_DIM:
        return "head_dim != 64"
    if cfg.hidden_act != "gelu":
        return f"hidden_act {cfg.hidden_act}"
    if c % 64 != 0 or c > rf.MAX_CHANNELS:
        return f"hidden size {c}"
    if getattr(cfg, "position_embedding_type", None) not in (None, "absolute"):
        return f"position_embedding_type {cfg.position_embedding_type}"
    if getattr(cfg, "is_decoder", False) or getattr(cfg, "add_cross_attention", False):
        return "decoder configuration"
    if text_backbone.pooler is None:
        return "no pooler"
    if input_ids.shape[1] > rf.MAX_KEYS:
        return f"more than {rf.MAX_KEYS} tokens"
    if torch.is_grad_enabled() and any(q.requires_grad for q in params):
        return "a parameter requires grad"
    if text_backbone.training and (cfg.hidden_dropout_prob > 0 or cfg.attention_probs_dropout_prob > 0):
        return "training-mode dropout"
    return None


def _stacked_qkv(layer):
    """(Wqkv [3C, C], bqkv [3C]) of one encoder layer, cached on the layer object."""
    att = layer.attention.self
    src = (att.query.weight, att.key.weight, att.value.weight, att.query.bias, att.key.bias, att.value.bias)
    key = tuple((t._version, t.data_ptr()) for t in src)
    cache = layer.__dict__.get(_CACHE_ATTR)
    if cache is None or cache[0] != key:
        with torch.no_grad():
            cache = (key, torch.cat([t.detach() for t in src[:3]], 0).contiguous(), torch.cat([t.detach() for t in src[3:]], 0).contiguous())
        layer.__dict__[_CACHE_ATTR] = cache              # a plain attribute: no parameter, no buffer, nothing in the state dict
    return cache[1], cache[2]


def validate(input_ids, attention_mask, vocab, pad_id, positions):
    """The checks the kernels rely on, on HOST tensors (what the tokenizer returned, before upload)."""
    if input_ids.dim() != 2 or input_ids.shape != attention_mask.shape:
        raise ValueError(f"roberta_forward: input_ids and attention_mask must be [B, L], got {tuple(input_ids.shape)}, {tuple(attention_mask.shape)}")
    l = input_ids.shape[1]
    if l + pad_id + 1 > positions:
        raise ValueError(f"roberta_forward: {l} tokens with pad id {pad_id} may need position {l + pad_id}, the table has {positions} rows")
    if input_ids.numel() and (int(input_ids.min()) < 0 or int(input_ids.max()) >= vocab):
        raise ValueError(f"roberta_forward: token id outside [0, {vocab})")
    if input_ids.numel() and not bool(attention_mask.ne(0).any(1).all()):
        raise ValueError("roberta_forward: an attention_mask row attends no key")


@torch.no_grad()
def roberta_forward(text_backbone, input_ids, attention_mask):
    """-> (last_hidden_state [B, L, C], pooler_output [B, C]) of `text_backbone` (HF RobertaModel) in fp32, on the device of its
    parameters.  input_ids / attention_mask [B, L] integer tensors; host tensors are validated for free and uploaded here, device
    tensors are read back once for the same checks.  The caller decides with `why_not` whether this path may serve the call."""
    cfg = text_backbone.config
    emb = text_backbone.embeddings
    dev = emb.word_embeddings.weight.device
    pad_id = int(emb.padding_idx if getattr(emb, "padding_idx", None) is not None else cfg.pad_token_id)
    validate(input_ids.cpu(), attention_mask.cpu(), emb.word_embeddings.weight.shape[0], pad_id, emb.position_embeddings.weight.shape[0])
    ids = input_ids.to(dev, torch.int64)
    attend = attention_mask.to(dev).ne(0).to(torch.uint8)
    b, l = ids.shape
    c, h, eps = cfg.hidden_size, cfg.num_attention_heads, cfg.layer_norm_eps
    with torch.autocast(device_type=dev.type, enabled=False):
        d = lambda t: t.detach()
        x = rf.embed_layer_norm(ids, d(emb.word_embeddings.weight), d(emb.position_embeddings.weight), d(emb.token_type_embeddings.weight)[0],
                                d(emb.LayerNorm.weight), d(emb.LayerNorm.bias), emb.LayerNorm.eps, pad_id).view(b * l, c)
        for layer in text_backbone.encoder.layer:
            wqkv, bqkv = _stacked_qkv(layer)
            a = rf.attention_hd64(rf.linear(x, wqkv, bqkv).view(b, l, 3 * c), attend, h).view(b * l, c)
            so, ff, fo = layer.attention.output, layer.intermediate.dense, layer.output
            x = rf.add_layer_norm(rf.linear(a, d(so.dense.weight), d(so.dense.bias)), x, d(so.LayerNorm.weight), d(so.LayerNorm.bias), eps)
            t = rf.linear(x, d(ff.weight))
            t = rf.bias_act(t, d(ff.bias), "gelu", out=t)
            x = rf.add_layer_norm(rf.linear(t, d(fo.dense.weight), d(fo.dense.bias)), x, d(fo.LayerNorm.weight), d(fo.LayerNorm.bias), eps)
        hidden = x.view(b, l, c)
        pool = text_backbone.pooler.dense
        pooled = rf.linear(hidden[:, 0].contiguous(), d(pool.weight))
        pooled = rf.bias_act(pooled, d(pool.bias), "tanh", out=pooled)
    return hidden, pooled


def encode(text_backbone, input_ids, attention_mask):
    """The switch-on route of TextEncoder._encode: the native forward where it serves, else HF through fallbacks.note (counted, warned
    once, an error under OCPG_STRICT_HIP=1; CPU parameters are the host-logic case and are not counted)."""
    reason = why_not(text_backbone, input_ids)
    if reason is None:
        return roberta_forward(text_backbone, input_ids, attention_mask)
    p = text_backbone.embeddings.word_embeddings.weight
    fallbacks.note("TextEncoder", f"native RoBERTa asked for, {reason}", p)
    enc = text_backbone(input_ids=input_ids.to(p.device), attention_mask=attention_mask.to(p.device))
    return enc.last_hidden_state, enc.pooler_output
