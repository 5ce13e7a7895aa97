"""Autograd binding of csrc/attn_smallk.hip and csrc/attn_longk.hip: multi-head attention against a short key sequence (the
vision-language fusion gate, models/segmentation.py:95-113, and the decoder's self-attention over its queries,
models/deformable_transformer.py:323-326).

`attention(q, k, v, key_padding_mask, scale, H, pdrop)` takes the projections' outputs as they are ([L, B, C] rows, any row
stride) and returns [Lq, B, C]; it returns None when the HIP kernels do not serve the shape (head_dim != 32, more than
`key_limit()` keys, ...) so that the caller keeps its generic path -- there is no silent fallback INSIDE this module.

Up to 32 keys run csrc/attn_smallk.hip (all K / V of a batch element in LDS); 33 .. MAX_KEYS keys run csrc/attn_longk.hip (keys in
chunks of 32; long captions: the reference tokenises with padding='longest' and no truncation).  OCPG_ATTN_LONGK=0 switches the
long-key kernels off (the library path of the caller serves more than 32 keys, as before them), =force serves every key count
the kernels can (LONGK_LIMIT) whatever MAX_KEYS says.
"""
import os

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from ...._lib import DTYPE_CODE as _DT, check, lib, stream_ptr
from .fused_ln_func import _unpack

SMALLK_KEYS = 32        # csrc/attn_smallk.hip
LONGK_LIMIT = 128       # csrc/attn_longk.hip
MAX_KEYS = 40           # most keys routed to the HIP kernels by default: the largest measured key count at which the long-key path is
                        # at least as fast as the library path from cold caches (1.19-1.32x at 40 keys,
                        # 0.96x at 64, 0.61x at 128 at the text gate's largest level)


def key_limit():
    """Most keys attention() serves now: MAX_KEYS, or what OCPG_ATTN_LONGK asks for (read per call: the A/B switch)."""
    mode = os.environ.get("OCPG_ATTN_LONGK", "1")
    return SMALLK_KEYS if mode == "0" else LONGK_LIMIT if mode == "force" else MAX_KEYS


def _rows(t):
    """[L, B, C] tensor whose rows (l, b) sit at (l * B + b) * ld: returns (tensor, ld), copying only if the view is not of that form."""
    if t.stride(-1) != 1 or (t.shape[0] > 1 and t.stride(0) != t.shape[1] * t.stride(1)) or t.stride(1) < t.shape[2]:
        t = t.contiguous()
    return t, t.stride(1)


def supported(q, k, H, pdrop):
    C = q.shape[-1]
    return (q.is_cuda and q.dtype in _DT and C % H == 0 and C // H == 32 and H <= 8 and 256 % H == 0 and k.shape[0] <= key_limit()
            and q.shape[1] <= 65535 and 0.0 <= pdrop < 1.0)


def _launches(batch_first, B, Lq, Lk, C, H):
    """The launches of one pass: per launch (batch entries it covers, element offsets of its q / out / dout / dq rows, k / v rows,
    padding row, lse rows, dk / dv rows).  Sequence-first is one launch over B; batch-first (q [B, Lq, C] against k / v [Lk, B, C]) is
    one launch per batch entry with B = 1 on the [L, 1, C] view of its rows."""
    if not batch_first:
        return [(B, 0, 0, 0, 0, 0)]
    return [(1, b * Lq * C, b * C, b * Lk, b * Lq * H, b * Lk * C) for b in range(B)]


def _at(t, offset):
    return None if t is None else t.data_ptr() + offset * t.element_size()


class ShortKeyAttention(Function):
    """Both kernel families (up to SMALLK_KEYS keys: csrc/attn_smallk.hip, more: csrc/attn_longk.hip) in both layouts.

    Sequence-first: q / k / v [L, B, C] with any row stride (`_rows`, no copy), dropout from (pdrop, rng).  Batch-first: q [B, Lq, C]
    (the visual tokens of the text gate are the channels-last feature map itself, [b, (t h w), c]; putting them token-major and back
    cost two transposing copies of the map each way), k / v stay [Lk, B, C] (row stride B * C per entry); no dropout.
    The long-key forward's output is kept for the backward: D = sum_j p~_j dp~_j = dout . out per (token, head), so the backward sweeps
    the key chunks once."""

    @staticmethod
    def forward(ctx, q, k, v, key_pad, scale, H, pdrop, rng, batch_first):
        if batch_first:
            q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
            B, Lq, C = q.shape
            ldq, ldk, ldv = C, B * C, B * C
        else:
            q, ldq = _rows(q)
            k, ldk = _rows(k)
            v, ldv = _rows(v)
            Lq, B, C = q.shape
        Lk = k.shape[0]
        pad = None if key_pad is None else key_pad.to(torch.uint8).contiguous()
        out = torch.empty(q.shape, dtype=q.dtype, device=q.device)
        lse = torch.empty(q.shape[:2] + (H,), dtype=torch.float32, device=q.device)
        seed, offset, base = (0, 0, None) if pdrop <= 0 else _unpack(rng)
        name = "ocpg_attn_smallk_fwd" if Lk <= SMALLK_KEYS else "ocpg_attn_longk_fwd"
        fn = getattr(lib(), name)
        with torch.cuda.device(q.device):
            for nb, oq, ok, op, ol, _ in _launches(batch_first, B, Lq, Lk, C, H):
                rc = fn(_at(q, oq), ldq, _at(k, ok), ldk, _at(v, ok), ldv, _at(pad, op), float(scale), Lq, nb, H, C // H, Lk, float(pdrop),
                        seed, offset, base, _at(out, oq), C, _at(lse, ol), _DT[q.dtype], stream_ptr())
                check(rc, name)
        ctx.save_for_backward(q, k, v, pad, lse, *((out,) if Lk > SMALLK_KEYS else ()))
        ctx.meta = (float(scale), H, float(pdrop), seed, offset, base, ldq, ldk, ldv, batch_first, B, Lq)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        q, k, v, pad, lse, *out = ctx.saved_tensors                 # out: the long-key path only
        scale, H, pdrop, seed, offset, base, ldq, ldk, ldv, batch_first, B, Lq = ctx.meta
        Lk, C = k.shape[0], q.shape[2]
        dout = dout.contiguous()
        dq = torch.empty(q.shape, dtype=q.dtype, device=q.device)
        dkv = torch.zeros((2, B, Lk, C) if batch_first else (2, Lk, B, C), dtype=torch.float32, device=q.device)
        dk, dv = dkv[0], dkv[1]
        name = "ocpg_attn_longk_bwd" if out else "ocpg_attn_smallk_bwd"
        fn = getattr(lib(), name)
        with torch.cuda.device(q.device):
            for nb, oq, ok, op, ol, od in _launches(batch_first, B, Lq, Lk, C, H):
                saved_out = (_at(out[0], oq), C) if out else ()
                rc = fn(_at(q, oq), ldq, _at(k, ok), ldk, _at(v, ok), ldv, _at(pad, op), _at(dout, oq), C, *saved_out, _at(lse, ol), scale,
                        Lq, nb, H, C // H, Lk, pdrop, seed, offset, base, _at(dq, oq), C, _at(dk, od), _at(dv, od), _DT[q.dtype],
                        stream_ptr())
                check(rc, name)
        if batch_first:
            dkv = dkv.transpose(1, 2)                               # [2, Lk, B, C]
        dkv = dkv.to(k.dtype)                                       # dk / dv accumulate in fp32 and are cast once
        return dq, dkv[0], dkv[1], None, None, None, None, None, None


def attention(q, k, v, key_padding_mask, scale, H, pdrop=0.0, rng=None):
    if not supported(q, k, H, pdrop):
        return None
    return ShortKeyAttention.apply(q, k, v, key_padding_mask, scale, H, pdrop, rng, False)


def attention_batch_first(q, k, v, key_padding_mask, scale, H):
    """q [B, Lq, C], k / v [Lk, B, C] -> [B, Lq, C]; None when the HIP kernels do not serve the shape."""
    if not (q.is_cuda and q.dtype in _DT and q.shape[-1] % H == 0 and q.shape[-1] // H == 32 and H <= 8 and 256 % H == 0
            and k.shape[0] <= key_limit()):
        return None
    return ShortKeyAttention.apply(q, k, v, key_padding_mask, scale, H, 0.0, None, True)
