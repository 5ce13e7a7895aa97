"""Autograd binding of csrc/text_gate.hip: the vision-language fusion gate (models/segmentation.py: VisionLanguageFusionModule) with its
query projection and out_proj folded into the text side.

    out[b, l, :] = x[b, l, :] * (out_proj(attention(q_proj(x[b, l, :]); k, v)))

With a handful of text keys, `q_proj` and `out_proj` reassociate onto the keys and values: per clip b, key k, head h

    K'[b, k, h, :] = Wq_h^T k[b,k,h,:]     c[b, k, h] = bq_h . k[b,k,h,:]     V'[b, k, h, :] = Wo[:, h-slice] v[b,k,h,:]

-- `text_operands` builds them with ordinary fp32 tensor ops (a few hundred kilobytes; autograd carries their gradients back to
in_proj_weight / in_proj_bias / out_proj and the text) ONCE per forward when the caller hands the same `shared` dict to the calls of
that forward: the model gates every pyramid level against the same text.
Everything per visual token is then one kernel forward (`ocpg_text_gate_fwd_h16`) and one call backward (`ocpg_text_gate_bwd_h16`).
By default only the backward is taken from the kernels and the forward stays the unfused path's, bit for bit (TextGateBackwardFunction);
OCPG_TEXT_GATE_FUSED=fwd runs the forward kernel too (its output differs from the unfused path's by 16-bit roundings).

`text_gate(...)` returns None when the kernels do not serve the call (not bf16 / fp16 autocast, more than 16 keys, another width or
head count, grad mode off, ...): the caller keeps its unfused path -- there is no silent fallback INSIDE this module.
"""
import os

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from ...._lib import H16_CODE as _DT, check, lib, stream_ptr

MODE = os.environ.get("OCPG_TEXT_GATE_FUSED", "1")                 # A/B switch, read once at import
ENABLED = MODE != "0"               # 0 = the unfused calls and autograd nodes
FUSED_FORWARD = MODE == "fwd"       # fwd = the forward through the kernel too; 1 (default): the forward keeps the unfused path's bits
MAX_KEYS = 16


class TextGateFunction(Function):
    """x [B, L, 256] fp32, Kp / Vp [B, 8 Lk, 256] fp32 (differentiable) with their 16-bit copies K16 / V16 (what the kernels read),
    c [B, 8 Lk] and bo [256] fp32, pad [B, Lk] uint8 or None -> out [B, L, 256] fp32."""

    @staticmethod
    def forward(ctx, x, Kp, Vp, c, bo, K16, V16, pad, scale, H):
        B, L, C = x.shape
        Lk = K16.shape[1] // H
        out = torch.empty_like(x)
        with torch.cuda.device(x.device):
            rc = lib().ocpg_text_gate_fwd_h16(x.data_ptr(), K16.data_ptr(), V16.data_ptr(), c.data_ptr(), bo.data_ptr(),
                                              None if pad is None else pad.data_ptr(), float(scale), B, L, C, H, Lk, out.data_ptr(),
                                              _DT[K16.dtype], stream_ptr())
        check(rc, "ocpg_text_gate_fwd_h16")
        ctx.save_for_backward(x, c, bo, K16, V16, pad)
        ctx.meta = (float(scale), H, Lk)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, c, bo, K16, V16, pad = ctx.saved_tensors
        return _backward(x, g, c, bo, K16, V16, pad, *ctx.meta) + (None,) * 5


def _backward(x, g, c, bo, K16, V16, pad, scale, H, Lk):
    """ocpg_text_gate_bwd_h16 -> (dx, dK', dV', dc, dbo)."""
    B, L, C = x.shape
    g = g.contiguous()
    NP, S = int(lib().ocpg_text_gate_rows(Lk)), int(lib().ocpg_text_gate_splits(L))
    N = H * Lk
    dx = torch.empty_like(x)
    part = torch.empty((S, B, 2 * NP * C + NP + C), dtype=torch.float32, device=x.device)
    ws = torch.empty((2, B, L, NP), dtype=K16.dtype, device=x.device)
    with torch.cuda.device(x.device):
        rc = lib().ocpg_text_gate_bwd_h16(x.data_ptr(), g.data_ptr(), K16.data_ptr(), V16.data_ptr(), c.data_ptr(), bo.data_ptr(),
                                          None if pad is None else pad.data_ptr(), scale, B, L, C, H, Lk, dx.data_ptr(), part.data_ptr(),
                                          ws.data_ptr(), _DT[K16.dtype], stream_ptr())
    check(rc, "ocpg_text_gate_bwd_h16")
    s = part.sum(0)                                                 # [B, W]: dK' | dV' | dc | dbo
    dK = s[:, :NP * C].view(B, NP, C)[:, :N]
    dV = s[:, NP * C:2 * NP * C].view(B, NP, C)[:, :N]
    dc = s[:, 2 * NP * C:2 * NP * C + N]
    dbo = s[:, 2 * NP * C + NP:].sum(0)
    return dx, dK, dV, dc, dbo


class TextGateBackwardFunction(Function):
    """The default: `out` [B, L, 256] is what the UNFUSED path computed from x (text_gate ran it on the detached map and dropped its
    autograd graph), so the output keeps the bits it always had -- the step is sensitive to the last bit of a forward activation
     -- and only the backward is the fused one: it needs x, g and the text-side operands, none of the unfused
    path's activations."""

    @staticmethod
    def forward(ctx, x, out, Kp, Vp, c, bo, K16, V16, pad, scale, H):
        ctx.save_for_backward(x, c, bo, K16, V16, pad)
        ctx.meta = (float(scale), H, K16.shape[1] // H)
        return out.detach()

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, c, bo, K16, V16, pad = ctx.saved_tensors
        dx, dK, dV, dc, dbo = _backward(x, g, c, bo, K16, V16, pad, *ctx.meta)
        return (dx, None, dK, dV, dc, dbo) + (None,) * 5


def text_operands(attn, key, value, low):
    """key / value [Lk, B, C] (the text with and without its position code) -> (K', V', c, bo, K16, V16): fp32 [B, 8 Lk, C], [B, 8 Lk, C],
    [B, 8 Lk], [C] and the `low`-precision copies of K' / V'.  Rows are key-major (n = key * H + head).  fp32 throughout, on the fp32
    parameters themselves (not their low-precision working copies)."""
    C, H = attn.embed_dim, attn.num_heads
    hd = C // H
    with torch.autocast("cuda", enabled=False):
        w, bias = attn.in_proj_weight, attn.in_proj_bias
        wq, wk, wv = w.chunk(3)
        bq, bk, bv = bias.chunk(3)
        Lk, B = key.shape[0], key.shape[1]
        k = torch.addmm(bk, key.float().reshape(Lk * B, C), wk.t()).view(Lk, B, H, hd).permute(1, 0, 2, 3)       # [B, Lk, H, hd]
        v = torch.addmm(bv, value.float().reshape(Lk * B, C), wv.t()).view(Lk, B, H, hd).permute(1, 0, 2, 3)
        # per head: K'[.., h, :] = k[.., h, :] Wq[h-slice, :],  V'[.., h, :] = v[.., h, :] Wo[:, h-slice]^T
        Kp = torch.einsum("bkhd,hdc->bkhc", k, wq.view(H, hd, C)).reshape(B, Lk * H, C).contiguous()
        Vp = torch.einsum("bkhd,chd->bkhc", v, attn.out_proj.weight.view(C, H, hd)).reshape(B, Lk * H, C).contiguous()
        c = torch.einsum("bkhd,hd->bkh", k, bq.view(H, hd)).reshape(B, Lk * H).contiguous()
        return Kp, Vp, c, attn.out_proj.bias, Kp.detach().to(low), Vp.detach().to(low)


def served(attn, visual, key):
    """The calls `text_gate` takes: a contiguous fp32 [B, L, 256] map on the GPU under bf16 / fp16 autocast, 8 heads, at most 16 keys,
    and a backward to come (grad mode on and the map, the text or a parameter of `attn` requires grad): the gate exists for its
    backward, and inference keeps the unfused calls and their bits."""
    return (ENABLED and visual.is_cuda and visual.dim() == 3 and visual.dtype == torch.float32 and visual.is_contiguous()
            and torch.is_autocast_enabled("cuda") and torch.get_autocast_dtype("cuda") in _DT
            and attn.embed_dim == 256 and attn.num_heads == 8 and 1 <= key.shape[0] <= MAX_KEYS and visual.shape[0] <= 65535
            and visual.data_ptr() % 16 == 0 and not (attn.training and attn.dropout > 0)
            and torch.is_grad_enabled() and (visual.requires_grad or key.requires_grad or attn.in_proj_weight.requires_grad
                                             or attn.out_proj.weight.requires_grad))


def text_gate(attn, visual, text, key_padding_mask, text_pos, unfused, shared=None):
    """visual [B, L, C] * attention of `attn` (a models.attention.MultiheadAttention) over text (+ text_pos) [Lk, B, C], or None when not
    served.  `unfused`: the unfused path as a function of the map; unless OCPG_TEXT_GATE_FUSED=fwd it computes the forward, and when it
    declines (None) so does this function.  `shared`: a dict the caller owns for ONE forward that gates several maps against the same
    text tensors; the text-side operands are built at the first call and kept there (with their autograd graph: the dict must not
    outlive the forward).  Without it every call builds its own."""
    if not served(attn, visual, text):
        return None
    out = None
    if not FUSED_FORWARD:
        out = unfused(visual.detach())          # grad mode is on (served): the routing, hence the GEMMs, of a training forward
        if out is None:
            return None
        out = out.detach()                      # its autograd graph is dropped here: the backward is the kernels'
    low = torch.get_autocast_dtype("cuda")
    tensors = (text, text_pos, key_padding_mask)
    hit = None if shared is None else shared.get("text_gate")
    if hit is None or hit[0] != low or any(a is not b for a, b in zip(hit[1], tensors)):
        key = text if text_pos is None else text + text_pos
        pad = None if key_padding_mask is None else key_padding_mask.to(torch.uint8).contiguous()
        hit = (low, tensors, text_operands(attn, key, text, low) + (pad,))
        if shared is not None:
            shared["text_gate"] = hit
    Kp, Vp, c, bo, K16, V16, pad = hit[2]
    scale, H = (attn.embed_dim // attn.num_heads) ** -0.5, attn.num_heads
    if FUSED_FORWARD:
        return TextGateFunction.apply(visual, Kp, Vp, c, bo, K16, V16, pad, scale, H)
    return TextGateBackwardFunction.apply(visual, out, Kp, Vp, c, bo, K16, V16, pad, scale, H)
