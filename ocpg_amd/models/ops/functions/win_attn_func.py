"""Fused (shifted-)window attention: autograd binding of ocpg_win_attn_{fwd,bwd} (csrc/win_attn.hip).

Replaces the score / bias / mask / softmax / PV chain of the reference's WindowAttention3D.forward
(models/video_swin_transformer.py:138-169).  What of size N x N reaches HBM besides the (tiny, per-head) relative-position bias and
its gradient depends on the path:
  * fp32 (csrc/win_attn.hip): nothing;
  * bf16 / fp16 through `window_attention` (the default): when the bias needs a gradient the matrix-core backward writes
    dS [BW, H, N, N] in the storage dtype (232 MB at Swin-T stage 1) and ATen sums it over the windows;
  * bf16 / fp16 through `window_attention_table` (opt-in, OCPG_WIN_ATTN_FUSED_DTABLE=1): nothing -- the backward returns the gradient
    of the relative-position TABLE, summed in LDS per (window, head); its only temporary is partials [BW, H, T] fp32.
"""
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from ...._lib import DTYPE_CODE as _DT, check, lib, stream_ptr


class WindowAttentionFunction(Function):
    @staticmethod
    def forward(ctx, qkv, bias, region, scale, num_windows, bias_t=None):
        """qkv [BW, N, 3, H, 32]; bias [H, N, N] (fp32); region [NW, N] int32 or None -> out [BW, N, H*32]."""
        if not qkv.is_cuda:
            raise RuntimeError("WindowAttentionFunction: qkv must be a GPU tensor: Not implemented on the CPU")
        if qkv.dtype not in _DT:
            raise RuntimeError(f"WindowAttentionFunction: unsupported dtype {qkv.dtype}")
        qkv = qkv.contiguous()
        bw, n, three, h, hd = qkv.shape
        assert three == 3
        bias = bias.float().contiguous()
        if bias_t is None or bias_t.dtype != torch.float32 or not bias_t.is_contiguous() or bias_t.shape != bias.shape:
            bias_t = bias.transpose(1, 2).contiguous()        # (models/video_swin_transformer.py hands the transposed table along: RelPosBias)
        out = torch.empty((bw, n, h * hd), dtype=qkv.dtype, device=qkv.device)
        lse = torch.empty((bw, h, n), dtype=torch.float32, device=qkv.device)
        with torch.cuda.device(qkv.device):
            check(lib().ocpg_win_attn_fwd(qkv.data_ptr(), bias_t.data_ptr(), region.data_ptr() if region is not None else None,
                                          float(scale), bw, int(num_windows), n, h, hd, out.data_ptr(), lse.data_ptr(),
                                          _DT[qkv.dtype], stream_ptr()), "ocpg_win_attn_fwd")
        ctx.save_for_backward(qkv, bias, bias_t, out, lse)
        ctx.region, ctx.scale, ctx.num_windows = region, float(scale), int(num_windows)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        qkv, bias, bias_t, out, lse = ctx.saved_tensors
        bw, n, _, h, hd = qkv.shape
        dout = dout.to(qkv.dtype).contiguous()
        dqkv = torch.empty_like(qkv)
        dbuf = torch.empty_like(lse)
        region = ctx.region
        if qkv.dtype != torch.float32:
            # matrix-core kernels (csrc/win_attn_mfma.hip): dS leaves as a [BW, H, N, N] tensor in the storage dtype and is summed
            # over the windows here (one streaming reduction instead of BW * H * N^2 float atomics)
            ds = torch.empty((bw, h, n, n), dtype=qkv.dtype, device=qkv.device) if ctx.needs_input_grad[1] else None
            with torch.cuda.device(qkv.device):
                rc = lib().ocpg_win_attn_bwd_mfma(qkv.data_ptr(), bias.data_ptr(), bias_t.data_ptr(),
                                                  region.data_ptr() if region is not None else None, ctx.scale, bw, ctx.num_windows, n, h, hd,
                                                  out.data_ptr(), dout.data_ptr(), lse.data_ptr(), dqkv.data_ptr(), dbuf.data_ptr(),
                                                  ds.data_ptr() if ds is not None else None, _DT[qkv.dtype], stream_ptr())
            if rc == 0:
                dbias = ds.sum(0, dtype=torch.float32).transpose(1, 2) if ds is not None else None
                return dqkv, dbias, None, None, None, None
            if rc != -2000:
                check(rc, "ocpg_win_attn_bwd_mfma")
        dbias_t = torch.zeros_like(bias_t) if ctx.needs_input_grad[1] else None
        with torch.cuda.device(qkv.device):
            check(lib().ocpg_win_attn_bwd(qkv.data_ptr(), bias.data_ptr(), bias_t.data_ptr(),
                                          region.data_ptr() if region is not None else None, ctx.scale, bw, ctx.num_windows, n, h, hd,
                                          out.data_ptr(), dout.data_ptr(), lse.data_ptr(), dqkv.data_ptr(), dbuf.data_ptr(),
                                          dbias_t.data_ptr() if dbias_t is not None else None, _DT[qkv.dtype], stream_ptr()),
                  "ocpg_win_attn_bwd")
        dbias = dbias_t.transpose(1, 2) if dbias_t is not None else None
        return dqkv, dbias, None, None, None, None


def window_attention(qkv, bias, region, scale, num_windows, bias_t=None):
    """bias_t (optional, no gradient): bias.transpose(1, 2) already contiguous."""
    return WindowAttentionFunction.apply(qkv, bias, region, scale, num_windows, bias_t)


def table_codes(index2d, cache=None):
    """Per-token codes of a relative-position index [n, n] (relative_position_index[:n, :n], the reference's slicing quirk kept):
    (tok_code int32 [n] on the index's device, code_off) with index2d[q, k] == tok_code[q] - tok_code[k] + code_off for every pair,
    or None when the index is not of that form.  The identity is verified against the whole index (one device round trip), so pass
    `cache`, a dict the owner of the index keeps (WindowAttention3D does): the check then runs once per (n, device)."""
    n = index2d.shape[0]
    key = (n, index2d.device)
    if cache is not None and key in cache:
        return cache[key]
    with torch.no_grad():
        idx = index2d.long()
        off = int(idx[0, 0])
        a = idx[:, 0] - off
        ok = tuple(index2d.shape) == (n, n) and bool(torch.equal(a[:, None] - a[None, :] + off, idx)) and bool(idx.min() >= 0)
        res = (a.to(torch.int32).contiguous(), off) if ok else None
    if cache is not None:
        cache[key] = res
    return res


class WindowAttentionTableFunction(Function):
    """Window attention whose differentiable inputs are qkv and the relative-position TABLE [T, H] (bf16 / fp16 storage, matrix-core
    kernels only).  Backward: ocpg_win_attn_bwd_mfma_dtable -- no dS tensor, no ATen sum, no relpos_bias_bwd."""

    @staticmethod
    def forward(ctx, qkv, table, index2d, region, scale, num_windows, codes):
        if not qkv.is_cuda:
            raise RuntimeError("WindowAttentionTableFunction: qkv must be a GPU tensor: Not implemented on the CPU")
        if qkv.dtype not in (torch.bfloat16, torch.float16):
            raise RuntimeError(f"WindowAttentionTableFunction: unsupported dtype {qkv.dtype} (bf16 / fp16 storage only)")
        qkv = qkv.contiguous()
        bw, n, three, h, hd = qkv.shape
        t = table.shape[0]
        assert three == 3 and table.shape[1] == h and tuple(index2d.shape) == (n, n)
        assert table.dtype == torch.float32 and table.is_contiguous() and index2d.dtype == torch.int64 and index2d.stride(1) == 1
        if codes is None:
            raise RuntimeError("WindowAttentionTableFunction: the index is not linear in a per-token code (table_codes returned None)")
        tok_code, code_off = codes
        if tok_code.shape[0] != n or tok_code.device != qkv.device or tok_code.dtype != torch.int32:
            raise RuntimeError("WindowAttentionTableFunction: token codes do not fit this window")
        if lib().ocpg_win_attn_dtable_supported(n, hd, _DT[qkv.dtype], t) != 1:
            raise RuntimeError(f"WindowAttentionTableFunction: N {n} / head_dim {hd} / T {t} not served by csrc/win_attn_mfma.hip")
        bias = torch.empty((h, n, n), dtype=torch.float32, device=qkv.device)
        bias_t = torch.empty_like(bias)
        out = torch.empty((bw, n, h * hd), dtype=qkv.dtype, device=qkv.device)
        lse = torch.empty((bw, h, n), dtype=torch.float32, device=qkv.device)
        with torch.cuda.device(qkv.device):
            check(lib().ocpg_relpos_bias_fwd(table.data_ptr(), index2d.data_ptr(), n, index2d.stride(0), h, bias.data_ptr(),
                                             bias_t.data_ptr(), stream_ptr()), "ocpg_relpos_bias_fwd")
            check(lib().ocpg_win_attn_fwd(qkv.data_ptr(), bias_t.data_ptr(), region.data_ptr() if region is not None else None,
                                          float(scale), bw, int(num_windows), n, h, hd, out.data_ptr(), lse.data_ptr(),
                                          _DT[qkv.dtype], stream_ptr()), "ocpg_win_attn_fwd")
        ctx.save_for_backward(qkv, bias, bias_t, out, lse, tok_code)
        ctx.region, ctx.scale, ctx.num_windows, ctx.code_off, ctx.rows = region, float(scale), int(num_windows), code_off, t
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        qkv, bias, bias_t, out, lse, tok_code = ctx.saved_tensors
        bw, n, _, h, hd = qkv.shape
        dout = dout.to(qkv.dtype).contiguous()
        dqkv = torch.empty_like(qkv)
        dbuf = torch.empty_like(lse)
        region = ctx.region.data_ptr() if ctx.region is not None else None
        with torch.cuda.device(qkv.device):
            if not ctx.needs_input_grad[1]:
                check(lib().ocpg_win_attn_bwd_mfma(qkv.data_ptr(), bias.data_ptr(), bias_t.data_ptr(), region, ctx.scale, bw, ctx.num_windows,
                                                   n, h, hd, out.data_ptr(), dout.data_ptr(), lse.data_ptr(), dqkv.data_ptr(),
                                                   dbuf.data_ptr(), None, _DT[qkv.dtype], stream_ptr()), "ocpg_win_attn_bwd_mfma")
                return dqkv, None, None, None, None, None, None
            partials = torch.empty((bw, h, ctx.rows), dtype=torch.float32, device=qkv.device)        # fully written by the kernel
            dtable = torch.empty((ctx.rows, h), dtype=torch.float32, device=qkv.device)
            check(lib().ocpg_win_attn_bwd_mfma_dtable(qkv.data_ptr(), bias.data_ptr(), bias_t.data_ptr(), region, ctx.scale, bw,
                                                      ctx.num_windows, n, h, hd, out.data_ptr(), dout.data_ptr(), lse.data_ptr(),
                                                      dqkv.data_ptr(), dbuf.data_ptr(), tok_code.data_ptr(), ctx.code_off, ctx.rows,
                                                      partials.data_ptr(), dtable.data_ptr(), _DT[qkv.dtype], stream_ptr()),
                  "ocpg_win_attn_bwd_mfma_dtable")
        return dqkv, dtable, None, None, None, None, None


def window_attention_table(qkv, table, index2d, region, scale, num_windows, codes=None):
    """qkv [BW, N, 3, H, 32] bf16 / fp16; table [T, H] fp32; index2d [N, N] int64 (relative_position_index[:N, :N]); region [NW, N] int32
    or None -> out [BW, N, H*32].  codes: table_codes(index2d) when the caller has it cached (computing it costs a device round trip)."""
    return WindowAttentionTableFunction.apply(qkv, table, index2d, region, scale, num_windows,
                                              codes if codes is not None else table_codes(index2d))
