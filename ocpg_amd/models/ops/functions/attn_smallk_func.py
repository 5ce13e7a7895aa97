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

from ...._lib import check, lib, stream_ptr
from .fused_ln_func import _unpack

_DT = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}
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


class SmallKeyAttention(Function):
    @staticmethod
    def forward(ctx, q, k, v, key_pad, scale, H, pdrop, rng):
        q, ldq = _rows(q)
        k, ldk = _rows(k)
        v, ldv = _rows(v)
        Lq, B, C = q.shape
        Lk = k.shape[0]
        pad = None if key_pad is None else key_pad.to(torch.uint8).contiguous()
        out = torch.empty((Lq, B, C), dtype=q.dtype, device=q.device)
        lse = torch.empty((Lq, B, H), dtype=torch.float32, device=q.device)
        seed, offset, base = (0, 0, None) if pdrop <= 0 else _unpack(rng)
        with torch.cuda.device(q.device):
            rc = lib().ocpg_attn_smallk_fwd(q.data_ptr(), ldq, k.data_ptr(), ldk, v.data_ptr(), ldv, None if pad is None else pad.data_ptr(),
                                            float(scale), Lq, B, H, C // H, Lk, float(pdrop), seed, offset, base, out.data_ptr(), C,
                                            lse.data_ptr(), _DT[q.dtype], stream_ptr())
        check(rc, "ocpg_attn_smallk_fwd")
        ctx.save_for_backward(q, k, v, pad, lse)
        ctx.meta = (float(scale), H, float(pdrop), seed, offset, base, ldq, ldk, ldv)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        q, k, v, pad, lse = ctx.saved_tensors
        scale, H, pdrop, seed, offset, base, ldq, ldk, ldv = ctx.meta
        Lq, B, C = q.shape
        Lk = k.shape[0]
        dout = dout.contiguous()
        dq = torch.empty((Lq, B, C), dtype=q.dtype, device=q.device)
        dkv = torch.zeros((2, Lk, B, C), dtype=torch.float32, device=q.device)
        with torch.cuda.device(q.device):
            rc = lib().ocpg_attn_smallk_bwd(q.data_ptr(), ldq, k.data_ptr(), ldk, v.data_ptr(), ldv, None if pad is None else pad.data_ptr(),
                                            dout.data_ptr(), C, lse.data_ptr(), scale, Lq, B, H, C // H, Lk, pdrop, seed, offset, base,
                                            dq.data_ptr(), C, dkv[0].data_ptr(), dkv[1].data_ptr(), _DT[q.dtype], stream_ptr())
        check(rc, "ocpg_attn_smallk_bwd")
        dkv = dkv.to(k.dtype)
        return dq, dkv[0], dkv[1], None, None, None, None, None


class LongKeyAttention(Function):
    """SmallKeyAttention for 33 .. 128 keys (csrc/attn_longk.hip).  The forward's output is kept for the backward: D = sum_j p~_j dp~_j
    = dout . out per (token, head), so the backward sweeps the key chunks once."""

    @staticmethod
    def forward(ctx, q, k, v, key_pad, scale, H, pdrop, rng):
        q, ldq = _rows(q)
        k, ldk = _rows(k)
        v, ldv = _rows(v)
        Lq, B, C = q.shape
        Lk = k.shape[0]
        pad = None if key_pad is None else key_pad.to(torch.uint8).contiguous()
        out = torch.empty((Lq, B, C), dtype=q.dtype, device=q.device)
        lse = torch.empty((Lq, B, H), dtype=torch.float32, device=q.device)
        seed, offset, base = (0, 0, None) if pdrop <= 0 else _unpack(rng)
        with torch.cuda.device(q.device):
            rc = lib().ocpg_attn_longk_fwd(q.data_ptr(), ldq, k.data_ptr(), ldk, v.data_ptr(), ldv, None if pad is None else pad.data_ptr(),
                                           float(scale), Lq, B, H, C // H, Lk, float(pdrop), seed, offset, base, out.data_ptr(), C,
                                           lse.data_ptr(), _DT[q.dtype], stream_ptr())
        check(rc, "ocpg_attn_longk_fwd")
        ctx.save_for_backward(q, k, v, pad, lse, out)
        ctx.meta = (float(scale), H, float(pdrop), seed, offset, base, ldq, ldk, ldv)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        q, k, v, pad, lse, out = ctx.saved_tensors
        scale, H, pdrop, seed, offset, base, ldq, ldk, ldv = ctx.meta
        Lq, B, C = q.shape
        Lk = k.shape[0]
        dout = dout.contiguous()
        dq = torch.empty((Lq, B, C), dtype=q.dtype, device=q.device)
        dkv = torch.zeros((2, Lk, B, C), dtype=torch.float32, device=q.device)
        with torch.cuda.device(q.device):
            rc = lib().ocpg_attn_longk_bwd(q.data_ptr(), ldq, k.data_ptr(), ldk, v.data_ptr(), ldv, None if pad is None else pad.data_ptr(),
                                           dout.data_ptr(), C, out.data_ptr(), C, lse.data_ptr(), scale, Lq, B, H, C // H, Lk, pdrop, seed,
                                           offset, base, dq.data_ptr(), C, dkv[0].data_ptr(), dkv[1].data_ptr(), _DT[q.dtype], stream_ptr())
        check(rc, "ocpg_attn_longk_bwd")
        dkv = dkv.to(k.dtype)
        return dq, dkv[0], dkv[1], None, None, None, None, None


def attention(q, k, v, key_padding_mask, scale, H, pdrop=0.0, rng=None):
    if not supported(q, k, H, pdrop):
        return None
    fn = SmallKeyAttention if k.shape[0] <= SMALLK_KEYS else LongKeyAttention
    return fn.apply(q, k, v, key_padding_mask, scale, H, pdrop, rng)


class SmallKeyAttentionBF(Function):
    """The same attention for queries stored BATCH-FIRST, q [B, Lq, C] (round 4: the visual tokens of the text gate are the channels-last
    feature map itself, [b, (t h w), c]; putting them token-major and back cost two transposing copies of the map each way).  One launch
    per batch entry on the [L, 1, C] view of its rows; k / v stay [Lk, B, C] (row stride B * C per entry, no copy).  No dropout."""

    @staticmethod
    def forward(ctx, q, k, v, key_pad, scale, H):
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        B, Lq, C = q.shape
        Lk = k.shape[0]
        pad = None if key_pad is None else key_pad.to(torch.uint8).contiguous()
        out = torch.empty((B, Lq, C), dtype=q.dtype, device=q.device)
        lse = torch.empty((B, Lq, H), dtype=torch.float32, device=q.device)
        es = q.element_size()
        with torch.cuda.device(q.device):
            for b in range(B):
                rc = lib().ocpg_attn_smallk_fwd(q.data_ptr() + b * Lq * C * es, C, k.data_ptr() + b * C * es, B * C, v.data_ptr() + b * C * es, B * C,
                                                None if pad is None else pad.data_ptr() + b * Lk, float(scale), Lq, 1, H, C // H, Lk, 0.0, 0, 0, None,
                                                out.data_ptr() + b * Lq * C * es, C, lse.data_ptr() + b * Lq * H * 4, _DT[q.dtype], stream_ptr())
                check(rc, "ocpg_attn_smallk_fwd")
        ctx.save_for_backward(q, k, v, pad, lse)
        ctx.meta = (float(scale), H)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        q, k, v, pad, lse = ctx.saved_tensors
        scale, H = ctx.meta
        B, Lq, C = q.shape
        Lk = k.shape[0]
        dout = dout.contiguous()
        dq = torch.empty((B, Lq, C), dtype=q.dtype, device=q.device)
        dkv = torch.zeros((2, B, Lk, C), dtype=torch.float32, device=q.device)
        es = q.element_size()
        with torch.cuda.device(q.device):
            for b in range(B):
                rc = lib().ocpg_attn_smallk_bwd(q.data_ptr() + b * Lq * C * es, C, k.data_ptr() + b * C * es, B * C, v.data_ptr() + b * C * es, B * C,
                                                None if pad is None else pad.data_ptr() + b * Lk, dout.data_ptr() + b * Lq * C * es, C,
                                                lse.data_ptr() + b * Lq * H * 4, scale, Lq, 1, H, C // H, Lk, 0.0, 0, 0, None,
                                                dq.data_ptr() + b * Lq * C * es, C, dkv[0, b].data_ptr(), dkv[1, b].data_ptr(), _DT[q.dtype],
                                                stream_ptr())
                check(rc, "ocpg_attn_smallk_bwd")
        dkv = dkv.transpose(1, 2).to(k.dtype)               # [2, Lk, B, C]
        return dq, dkv[0], dkv[1], None, None, None


class LongKeyAttentionBF(Function):
    """SmallKeyAttentionBF for 33 .. 128 keys (csrc/attn_longk.hip): one launch per batch entry each way, the forward's output kept."""

    @staticmethod
    def forward(ctx, q, k, v, key_pad, scale, H):
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        B, Lq, C = q.shape
        Lk = k.shape[0]
        pad = None if key_pad is None else key_pad.to(torch.uint8).contiguous()
        out = torch.empty((B, Lq, C), dtype=q.dtype, device=q.device)
        lse = torch.empty((B, Lq, H), dtype=torch.float32, device=q.device)
        es = q.element_size()
        with torch.cuda.device(q.device):
            for b in range(B):
                rc = lib().ocpg_attn_longk_fwd(q.data_ptr() + b * Lq * C * es, C, k.data_ptr() + b * C * es, B * C, v.data_ptr() + b * C * es, B * C,
                                               None if pad is None else pad.data_ptr() + b * Lk, float(scale), Lq, 1, H, C // H, Lk, 0.0, 0, 0, None,
                                               out.data_ptr() + b * Lq * C * es, C, lse.data_ptr() + b * Lq * H * 4, _DT[q.dtype], stream_ptr())
                check(rc, "ocpg_attn_longk_fwd")
        ctx.save_for_backward(q, k, v, pad, lse, out)
        ctx.meta = (float(scale), H)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        q, k, v, pad, lse, out = ctx.saved_tensors
        scale, H = ctx.meta
        B, Lq, C = q.shape
        Lk = k.shape[0]
        dout = dout.contiguous()
        dq = torch.empty((B, Lq, C), dtype=q.dtype, device=q.device)
        dkv = torch.zeros((2, B, Lk, C), dtype=torch.float32, device=q.device)
        es = q.element_size()
        with torch.cuda.device(q.device):
            for b in range(B):
                rc = lib().ocpg_attn_longk_bwd(q.data_ptr() + b * Lq * C * es, C, k.data_ptr() + b * C * es, B * C, v.data_ptr() + b * C * es, B * C,
                                               None if pad is None else pad.data_ptr() + b * Lk, dout.data_ptr() + b * Lq * C * es, C,
                                               out.data_ptr() + b * Lq * C * es, C, lse.data_ptr() + b * Lq * H * 4, scale, Lq, 1, H, C // H, Lk,
                                               0.0, 0, 0, None, dq.data_ptr() + b * Lq * C * es, C, dkv[0, b].data_ptr(), dkv[1, b].data_ptr(),
                                               _DT[q.dtype], stream_ptr())
                check(rc, "ocpg_attn_longk_bwd")
        dkv = dkv.transpose(1, 2).to(k.dtype)               # [2, Lk, B, C]
        return dq, dkv[0], dkv[1], None, None, None


def attention_batch_first(q, k, v, key_padding_mask, scale, H):
    """q [B, Lq, C], k / v [Lk, B, C] -> [B, Lq, C]; None when the HIP kernels do not serve the shape."""
    if not (q.is_cuda and q.dtype in _DT and q.shape[-1] % H == 0 and q.shape[-1] // H == 32 and H <= 8 and 256 % H == 0
            and k.shape[0] <= key_limit()):
        return None
    fn = SmallKeyAttentionBF if k.shape[0] <= SMALLK_KEYS else LongKeyAttentionBF
    return fn.apply(q, k, v, key_padding_mask, scale, H)
