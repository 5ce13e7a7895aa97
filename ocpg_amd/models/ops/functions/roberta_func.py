"""Bindings of the text-encoder kernels (csrc/roberta.hip): ocpg_roberta_embed_ln_f32, ocpg_attn_hd64_fwd_f32, ocpg_bias_act_f32, and
the two library entry points the encoder's runner strings between them (`linear`: ocpg_small_linear_f32_fwd / ocpg_gemm; `add_layer_norm`:
ocpg_dropout_add_ln_fwd at p = 0).  fp32, forward only: every function raises when an input requires grad.  GPU tensors run the HIP
kernels; CPU tensors run a torch composition of the same arithmetic, so the runner (models/text_encoder/roberta_native.py) and the host
logic stay testable without a GPU.
"""
import os

import torch
import torch.nn.functional as F

from ...._lib import check, lib, stream_ptr

HEAD_DIM = 64
MAX_KEYS = 128              # csrc/roberta.hip: MAXL
MAX_CHANNELS = 1024         # embed_layer_norm: 4 float4 per lane
ACTS = {"none": 0, "gelu": 1, "tanh": 2}
# which entry point serves a dense product of R rows: "auto" = the few-row exact-fp32 MFMA kernel up to SMALL_ROWS rows, the planned
# library GEMM beyond; "small" / "gemm" force one (the A/B tool's switch).  Measured (tools/text_native_ab.py): at
# R = 8 .. 80 ocpg_gemm takes 21 us per call on all four layer shapes (the host's issue rate), the few-row kernel 27-30 us on the three
# 768-deep shapes and 97-108 us on the 3072-deep one (12 workgroups walking 48 K steps) -- so no row count goes to it: SMALL_ROWS = 0
ROUTE = os.environ.get("OCPG_TEXT_GEMM", "auto")
SMALL_ROWS = 0


def _no_grad(name, *tensors):
    for t in tensors:
        if t is not None and t.requires_grad:
            raise RuntimeError(f"{name}: forward only -- an input requires grad")


def _f32(name, *tensors):
    for t in tensors:
        if t is not None and t.dtype != torch.float32:
            raise ValueError(f"{name}: fp32 tensors only, got {t.dtype}")


def position_ids(ids, pad_id):
    """HF's create_position_ids_from_input_ids: pad + the running count of non-pad tokens, pad at a pad token (host / composition form)."""
    nonpad = ids.ne(pad_id)
    return torch.cumsum(nonpad.to(torch.int64), 1) * nonpad.to(torch.int64) + pad_id


def embed_layer_norm(ids, word, pos, type0, gamma, beta, eps, pad_id, bad=None):
    """ids int64 [B, L] -> LayerNorm(word[ids] + type0 + pos[position ids]) [B, L, C] fp32; type0 [C] is row 0 of the token-type table.
    L + pad_id + 1 > P raises before any launch.  bad: None, or an int32 [1] counter (zeroed by the caller) that receives the number of
    ids outside [0, V); such a token's word row is zeros.  Without `bad`, CPU ids outside the range raise; GPU ids are not read back
    (the kernel still reads nothing out of bounds)."""
    _no_grad("embed_layer_norm", word, pos, type0, gamma, beta)
    _f32("embed_layer_norm", word, pos, type0, gamma, beta)
    if ids.dim() != 2 or ids.dtype != torch.int64:
        raise ValueError(f"embed_layer_norm: ids must be int64 [B, L], got {ids.dtype} {tuple(ids.shape)}")
    b, l = ids.shape
    v, c = word.shape
    p = pos.shape[0]
    pad_id = int(pad_id)
    if pos.shape[1] != c or type0.shape != (c,) or gamma.shape != (c,) or beta.shape != (c,):
        raise ValueError("embed_layer_norm: the tables and the LayerNorm parameters must share the channel count")
    if c % 4 != 0 or c > MAX_CHANNELS:
        raise ValueError(f"embed_layer_norm: C % 4 == 0 and C <= {MAX_CHANNELS} are served, got {c}")
    if pad_id < 0 or l + pad_id + 1 > p:
        raise ValueError(f"embed_layer_norm: {l} tokens with pad id {pad_id} may need position {l + pad_id}, the table has {p} rows")
    if not ids.is_cuda:
        ok = (ids >= 0) & (ids < v)
        if bad is None:
            if not bool(ok.all()):
                raise ValueError(f"embed_layer_norm: token id outside [0, {v})")
        else:
            bad += int((~ok).sum())
        w = word[ids.clamp(0, v - 1)] * ok[..., None].to(word.dtype)
        z = (w + type0) + pos[position_ids(ids, pad_id)]
        return F.layer_norm(z, (c,), gamma, beta, eps)
    ids = ids.contiguous()
    word, pos, type0, gamma, beta = (t.contiguous() for t in (word, pos, type0, gamma, beta))
    out = torch.empty((b, l, c), dtype=torch.float32, device=ids.device)
    with torch.cuda.device(ids.device):
        check(lib().ocpg_roberta_embed_ln_f32(ids.data_ptr(), word.data_ptr(), pos.data_ptr(), type0.data_ptr(), gamma.data_ptr(),
                                              beta.data_ptr(), float(eps), pad_id, b, l, c, v, p, out.data_ptr(),
                                              None if bad is None else bad.data_ptr(), stream_ptr()), "ocpg_roberta_embed_ln_f32")
    return out


def attention_hd64(qkv, attend, heads, scale=None):
    """qkv [B, L, 3 * heads * 64] (or [B, L, 3, heads, 64]): the stacked q / k / v projection; attend [B, L] uint8 / bool / int64,
    non-zero = the key is attended -> softmax(q k^T scale + mask) v as [B, L, heads * 64].  Every row must attend a key (the caller's
    check, on the host tensors).  1 <= L <= 128."""
    _no_grad("attention_hd64", qkv)
    _f32("attention_hd64", qkv)
    b, l = qkv.shape[:2]
    h = int(heads)
    if qkv.numel() != b * l * 3 * h * HEAD_DIM:
        raise ValueError(f"attention_hd64: expected [B, L, 3 * {h} * {HEAD_DIM}], got {tuple(qkv.shape)}")
    if tuple(attend.shape) != (b, l):
        raise ValueError(f"attention_hd64: attend must be [B, L] = {(b, l)}, got {tuple(attend.shape)}")
    if not 1 <= l <= MAX_KEYS:
        raise ValueError(f"attention_hd64: 1 to {MAX_KEYS} keys are served, got {l}")
    scale = HEAD_DIM ** -0.5 if scale is None else float(scale)
    if attend.dtype == torch.bool:
        attend = attend.to(torch.uint8)
    if attend.dtype not in (torch.uint8, torch.int64):
        raise ValueError(f"attention_hd64: attend must be uint8, bool or int64, got {attend.dtype}")
    if not qkv.is_cuda:
        q, k, v = qkv.reshape(b, l, 3, h, HEAD_DIM).permute(2, 0, 3, 1, 4)                    # [B, H, L, 64] each
        s = (q @ k.transpose(-1, -2)) * scale
        s = s.masked_fill(attend.to(qkv.device).eq(0)[:, None, None, :], float("-inf"))
        return (torch.softmax(s, -1) @ v).permute(0, 2, 1, 3).reshape(b, l, h * HEAD_DIM)
    qkv, attend = qkv.contiguous(), attend.contiguous()
    out = torch.empty((b, l, h * HEAD_DIM), dtype=torch.float32, device=qkv.device)
    with torch.cuda.device(qkv.device):
        check(lib().ocpg_attn_hd64_fwd_f32(qkv.data_ptr(), attend.data_ptr(), int(attend.dtype == torch.int64), scale, b, l, h, out.data_ptr(),
                                           stream_ptr()), "ocpg_attn_hd64_fwd_f32")
    return out


def bias_act(x, bias, act, out=None):
    """act(x + bias) over the last axis of a contiguous x; bias [C] or None; act "none" | "gelu" (exact, erf) | "tanh"; out may be x."""
    _no_grad("bias_act", x, bias)
    _f32("bias_act", x, bias)
    if act not in ACTS:
        raise ValueError(f"bias_act: act must be one of {sorted(ACTS)}, got {act!r}")
    c = x.shape[-1]
    if bias is not None and tuple(bias.shape) != (c,):
        raise ValueError(f"bias_act: bias must be [{c}], got {tuple(bias.shape)}")
    if not x.is_contiguous():
        raise ValueError("bias_act: x has to be contiguous")
    if out is None:
        out = torch.empty_like(x)
    elif out.shape != x.shape or out.dtype != x.dtype or out.device != x.device or not out.is_contiguous():
        raise ValueError("bias_act: out must match x")
    if not x.is_cuda:
        z = x if bias is None else x + bias
        out.copy_(F.gelu(z) if act == "gelu" else torch.tanh(z) if act == "tanh" else z)
        return out
    if x.numel():
        with torch.cuda.device(x.device):
            check(lib().ocpg_bias_act_f32(x.data_ptr(), None if bias is None else bias.contiguous().data_ptr(), x.numel() // c, c, ACTS[act],
                                          out.data_ptr(), stream_ptr()), "ocpg_bias_act_f32")
    return out


def linear(x2, w, b=None, route=None):
    """x2 [R, K] @ w [N, K]^T (+ b) in fp32: the few-row exact-fp32 MFMA kernel or the planned library GEMM (ROUTE / SMALL_ROWS)."""
    _no_grad("linear", x2, w, b)
    _f32("linear", x2, w, b)
    if not x2.is_cuda:
        return F.linear(x2, w, b)
    route = route or ROUTE
    r, k = x2.shape
    n = w.shape[0]
    x2, w = x2.contiguous(), w.contiguous()
    if route == "small" or (route == "auto" and r <= SMALL_ROWS and k % 64 == 0):
        y = torch.empty((r, n), dtype=torch.float32, device=x2.device)
        with torch.cuda.device(x2.device):
            check(lib().ocpg_small_linear_f32_fwd(x2.data_ptr(), w.data_ptr(), None if b is None else b.data_ptr(), r, k, n, y.data_ptr(),
                                                  stream_ptr()), "ocpg_small_linear_f32_fwd")
        return y
    from .gemm_func import gemm
    with torch.cuda.device(x2.device):
        return gemm(x2, w, False, True, b)


def add_layer_norm(x2, res2, gamma, beta, eps):
    """LayerNorm(res2 + x2) over [R, C]: the dropout + add + LayerNorm kernel at p = 0 (csrc/fused_ln.hip)."""
    _no_grad("add_layer_norm", x2, res2, gamma, beta)
    _f32("add_layer_norm", x2, res2, gamma, beta)
    r, c = x2.shape
    if not x2.is_cuda:
        return F.layer_norm(res2 + x2, (c,), gamma, beta, eps)
    y = torch.empty((r, c), dtype=torch.float32, device=x2.device)
    stats = torch.empty((2, r), dtype=torch.float32, device=x2.device)
    with torch.cuda.device(x2.device):
        check(lib().ocpg_dropout_add_ln_fwd(x2.data_ptr(), res2.data_ptr(), gamma.data_ptr(), beta.data_ptr(), r, c, float(eps), 0.0, 0, 0, None, 0,
                                            y.data_ptr(), stats[0].data_ptr(), stats[1].data_ptr(), stream_ptr()), "ocpg_dropout_add_ln_fwd")
    return y
