"""MSDeformAttnFunction -- autograd binding of the HIP op; mirrors the reference's
models/ops/functions/ms_deform_attn_func.py:21-39 (same ``apply`` signature, same saved tensors, same
returned gradient tuple) but calls libocpg_hip.so through its C ABI instead of the pybind CUDA module.

Error behaviour follows ms_deform_attn_cuda.cu:28-38 / ms_deform_attn.h:38,60: non-contiguous or CPU tensors
raise RuntimeError.  ``im2col_step`` is accepted and ignored (no chunking, hence no ``N % step`` restriction).
"""
import ctypes

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from ...._lib import H16_CODE as _H16, check, lib, require_gpu, stream_ptr      # _H16: 16-bit STORAGE of value / out / grad_out (ocpg_msda_*_h16)


# -- optional live kernel timing (bench.py): events on the launch stream around every kernel call -----------------
_TIMING = {"on": False, "events": []}


def enable_kernel_timing(on=True):
    _TIMING["on"] = on
    _TIMING["events"] = []


def collect_kernel_timing():
    """-> {"fwd_enc": {"ms": total, "n": launches}, ...}; 'enc' = self-attention shape (Lq == S), else 'dec'."""
    torch.cuda.synchronize()
    out = {}
    for key, e0, e1 in _TIMING["events"]:
        d = out.setdefault(key, {"ms": 0.0, "n": 0})
        d["ms"] += e0.elapsed_time(e1)
        d["n"] += 1
    _TIMING["events"] = []
    _TIMING["on"] = False
    return out


class _timed:
    def __init__(self, key):
        self.key = key

    def __enter__(self):
        if _TIMING["on"]:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e1 = torch.cuda.Event(enable_timing=True)
            self.e0.record()

    def __exit__(self, *exc):
        if _TIMING["on"]:
            self.e1.record()
            _TIMING["events"].append((self.key, self.e0, self.e1))


def _host_shapes(spatial_shapes):
    """Host copy of the [L,2] shapes tensor. Our own transformer attaches it (no sync); foreign callers pay one
    D2H copy -- the reference's module syncs on the same tensor anyway (ms_deform_attn.py:94 assert)."""
    hs = getattr(spatial_shapes, "_ocpg_host", None)
    if hs is None:
        hs = spatial_shapes.detach().cpu().contiguous()
    return hs


def _dims(value, loc):
    N, S, M, D = value.shape
    _, Lq, _, L, P, _ = loc.shape
    return N, S, M, D, L, Lq, P


def _check_h16(fn, value, sampling_loc, attn_weight):
    """a 16-bit value needs fp32 sampling locations and attention weights (coordinates do not survive 8 mantissa bits)"""
    for n, t in (("sampling_loc", sampling_loc), ("attn_weight", attn_weight)):
        if t.dtype != torch.float32:
            raise RuntimeError(f"{fn}: with a {value.dtype} value, {n} must be float32 (got {t.dtype})")


def ms_deform_attn_forward(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, im2col_step=64):
    for n, t in (("value", value), ("spatial_shapes", spatial_shapes), ("level_start_index", level_start_index),
                 ("sampling_loc", sampling_loc), ("attn_weight", attn_weight)):
        require_gpu(n, t)
    if value.dtype in _H16:
        _check_h16("ms_deform_attn_forward", value, sampling_loc, attn_weight)
        if spatial_shapes.dtype != torch.int64 or level_start_index.dtype != torch.int64:
            raise RuntimeError("ms_deform_attn_forward: spatial_shapes / level_start_index must be int64")
        N, S, M, D, L, Lq, P = _dims(value, sampling_loc)
        out = torch.empty((N, Lq, M * D), dtype=value.dtype, device=value.device)
        with torch.cuda.device(value.device), _timed("fwd_enc" if Lq == S else "fwd_dec"):
            check(lib().ocpg_msda_fwd_h16(value.data_ptr(), spatial_shapes.data_ptr(), level_start_index.data_ptr(),
                                          sampling_loc.data_ptr(), attn_weight.data_ptr(), N, S, M, D, L, Lq, P, out.data_ptr(),
                                          None, _H16[value.dtype], stream_ptr()), "ocpg_msda_fwd_h16")
        return out
    if value.dtype not in (torch.float32, torch.float64):
        raise RuntimeError("ms_deform_attn_forward: only float32 / float64 (and bfloat16 / float16 storage of value) are supported")
    if sampling_loc.dtype != value.dtype or attn_weight.dtype != value.dtype:
        raise RuntimeError("ms_deform_attn_forward: value / sampling_loc / attn_weight dtypes differ")
    if spatial_shapes.dtype != torch.int64 or level_start_index.dtype != torch.int64:
        raise RuntimeError("ms_deform_attn_forward: spatial_shapes / level_start_index must be int64")
    N, S, M, D, L, Lq, P = _dims(value, sampling_loc)
    out = torch.empty((N, Lq, M * D), dtype=value.dtype, device=value.device)
    with torch.cuda.device(value.device), _timed("fwd_enc" if Lq == S else "fwd_dec"):
        if value.dtype == torch.float32:
            # only the opt-in LDS-window forward reads it: never pay a device-to-host copy for it
            hs = getattr(spatial_shapes, "_ocpg_host", None) if Lq == S else None
            check(lib().ocpg_msda_fwd_f32(value.data_ptr(), spatial_shapes.data_ptr(), level_start_index.data_ptr(),
                                          sampling_loc.data_ptr(), attn_weight.data_ptr(), N, S, M, D, L, Lq, P, out.data_ptr(),
                                          ctypes.c_void_p(hs.data_ptr()) if hs is not None else None, stream_ptr()),
                  "ocpg_msda_fwd")
        else:
            check(lib().ocpg_msda_fwd_f64(value.data_ptr(), spatial_shapes.data_ptr(), level_start_index.data_ptr(),
                                          sampling_loc.data_ptr(), attn_weight.data_ptr(), N, S, M, D, L, Lq, P, out.data_ptr(),
                                          stream_ptr()), "ocpg_msda_fwd")
    return out


def ms_deform_attn_backward(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, grad_output, im2col_step=64, sel_state=None):
    """sel_state: the call site's path-selection state (int32[8] on the device, zero-filled once; include/ocpg_hip.h
    ocpg_msda_bwd_value_sel_f32) or None for the fixed default path."""
    for n, t in (("value", value), ("spatial_shapes", spatial_shapes), ("level_start_index", level_start_index),
                 ("sampling_loc", sampling_loc), ("attn_weight", attn_weight), ("grad_output", grad_output)):
        require_gpu(n, t)
    N, S, M, D, L, Lq, P = _dims(value, sampling_loc)
    if value.dtype in _H16:
        # whole backward behind one entry point; grad_value is accumulated in fp32 (no 16-bit atomics) and handed back in value's dtype
        _check_h16("ms_deform_attn_backward", value, sampling_loc, attn_weight)
        if grad_output.dtype != value.dtype:
            raise RuntimeError(f"ms_deform_attn_backward: grad_output must have value's dtype {value.dtype} (got {grad_output.dtype})")
        grad_value = torch.zeros(value.shape, dtype=torch.float32, device=value.device)
        grad_loc = torch.empty_like(sampling_loc)
        grad_attn = torch.empty_like(attn_weight)
        hs = _host_shapes(spatial_shapes) if Lq == S else None
        with torch.cuda.device(value.device), _timed("bwd_enc" if Lq == S else "bwd_dec"):
            check(lib().ocpg_msda_bwd_h16(value.data_ptr(), spatial_shapes.data_ptr(), level_start_index.data_ptr(),
                                          sampling_loc.data_ptr(), attn_weight.data_ptr(), grad_output.data_ptr(),
                                          N, S, M, D, L, Lq, P, grad_value.data_ptr(), grad_loc.data_ptr(), grad_attn.data_ptr(),
                                          ctypes.c_void_p(hs.data_ptr()) if hs is not None else None,
                                          sel_state.data_ptr() if sel_state is not None else None, _H16[value.dtype], stream_ptr()),
                  "ocpg_msda_bwd_h16")
        return grad_value.to(value.dtype), grad_loc, grad_attn
    grad_value = torch.zeros_like(value)
    grad_loc = torch.empty_like(sampling_loc)
    grad_attn = torch.empty_like(attn_weight)
    if value.dtype == torch.float32 and Lq == S:
        # self-attention: the two halves of the backward are separate kernels behind their own entry points (timed apart)
        hs = _host_shapes(spatial_shapes)
        L_ = lib()
        with torch.cuda.device(value.device):
            with _timed("bwd_enc_value"):
                if sel_state is not None:
                    rc1 = L_.ocpg_msda_bwd_value_sel_f32(sampling_loc.data_ptr(), attn_weight.data_ptr(), grad_output.data_ptr(), N, S, M, D, L,
                                                         Lq, P, grad_value.data_ptr(), ctypes.c_void_p(hs.data_ptr()), sel_state.data_ptr(),
                                                         stream_ptr())
                else:
                    rc1 = L_.ocpg_msda_bwd_value_f32(sampling_loc.data_ptr(), attn_weight.data_ptr(), grad_output.data_ptr(), N, S, M, D, L,
                                                     Lq, P, grad_value.data_ptr(), ctypes.c_void_p(hs.data_ptr()), stream_ptr())
            if rc1 == 0:
                with _timed("bwd_enc_locattn"):
                    rc2 = L_.ocpg_msda_bwd_locattn_f32(value.data_ptr(), spatial_shapes.data_ptr(), level_start_index.data_ptr(),
                                                       sampling_loc.data_ptr(), attn_weight.data_ptr(), grad_output.data_ptr(), N, S,
                                                       M, D, L, Lq, P, grad_loc.data_ptr(), grad_attn.data_ptr(), stream_ptr())
                check(rc2, "ocpg_msda_bwd_locattn")
                return grad_value, grad_loc, grad_attn
            if rc1 != -2000:
                check(rc1, "ocpg_msda_bwd_value")
    with torch.cuda.device(value.device), _timed("bwd_enc" if Lq == S else "bwd_dec"):
        if value.dtype == torch.float32:
            hs = _host_shapes(spatial_shapes) if Lq == S else None
            check(lib().ocpg_msda_bwd_f32(value.data_ptr(), spatial_shapes.data_ptr(), level_start_index.data_ptr(),
                                          sampling_loc.data_ptr(), attn_weight.data_ptr(), grad_output.data_ptr(),
                                          N, S, M, D, L, Lq, P, grad_value.data_ptr(), grad_loc.data_ptr(),
                                          grad_attn.data_ptr(), ctypes.c_void_p(hs.data_ptr()) if hs is not None else None,
                                          stream_ptr()), "ocpg_msda_bwd")
        elif value.dtype == torch.float64:
            check(lib().ocpg_msda_bwd_f64(value.data_ptr(), spatial_shapes.data_ptr(), level_start_index.data_ptr(),
                                          sampling_loc.data_ptr(), attn_weight.data_ptr(), grad_output.data_ptr(),
                                          N, S, M, D, L, Lq, P, grad_value.data_ptr(), grad_loc.data_ptr(),
                                          grad_attn.data_ptr(), stream_ptr()), "ocpg_msda_bwd")
        else:
            raise RuntimeError("ms_deform_attn_backward: only float32 / float64 (and bfloat16 / float16 storage of value) are supported")
    return grad_value, grad_loc, grad_attn


class MSDeformAttnFunction(Function):
    @staticmethod
    def forward(ctx, value, value_spatial_shapes, value_level_start_index, sampling_locations, attention_weights, im2col_step):
        ctx.im2col_step = im2col_step
        output = ms_deform_attn_forward(value, value_spatial_shapes, value_level_start_index, sampling_locations,
                                        attention_weights, im2col_step)
        ctx.save_for_backward(value, value_spatial_shapes, value_level_start_index, sampling_locations, attention_weights)
        ctx.shapes_host = getattr(value_spatial_shapes, "_ocpg_host", None)
        ctx.sel_state = getattr(sampling_locations, "_ocpg_sel", None)       # the calling module's path-selection state (or None)
        return output

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        value, shapes, level_start, loc, attn = ctx.saved_tensors
        if ctx.shapes_host is not None:
            shapes._ocpg_host = ctx.shapes_host
        gv, gl, ga = ms_deform_attn_backward(value, shapes, level_start, loc, attn, grad_output.contiguous(), ctx.im2col_step, ctx.sel_state)
        return gv, None, None, gl, ga, None


class MSDeformAttnFusedFunction(Function):
    """The module's front end fused into the op (include/ocpg_hip.h: ocpg_msda_fused_fwd_f32 / _bwd_qproj_f32 and their _h16 forms): softmax
    over the L*P logits and `reference + offset` (ms_deform_attn.py:96-110, 2-d reference branch) inside the forward kernel's sample setup,
    the softmax backward and the [d offsets | d logits] layout inside the gather kernel's epilogue.  Self-attention calls only (Lq == S),
    D = 32, L*P = 16, reference points without gradient; `supported()` says whether a call qualifies -- the module keeps the unfused path
    otherwise.
    value is float32, or bfloat16 / float16 (16-bit STORAGE of value / out / grad_out): qproj, ref and the returned loc / attn are float32
    in every case, out has value's dtype, grad_output must arrive in value's dtype, grad_value is accumulated in an fp32 buffer and
    handed back in value's dtype.  A 16-bit call the fused kernels decline (-2000: a buffer off the alignment their vector accesses need)
    is served by the un-fused 16-bit entry points with the front end in torch: same results, no exception.

    apply(value [N,S,M,D], shapes, level_start, qproj [N,Lq,3*M*L*P], ref [N,Lq,L,2], L, P, sel_state) -> (out, loc, attn)"""

    @staticmethod
    def supported(value, qproj, ref, L, P):
        return (value.is_cuda and (value.dtype == torch.float32 or value.dtype in _H16) and qproj.dtype == torch.float32
                and ref.dtype == torch.float32 and value.shape[-1] == 32 and L * P == 16 and ref.shape[-1] == 2 and not ref.requires_grad
                and value.shape[1] == qproj.shape[1] and qproj.is_contiguous())

    @staticmethod
    def forward(ctx, value, shapes, level_start, qproj, ref, L, P, sel_state):
        N, S, M, D = value.shape
        Lq = qproj.shape[1]
        value, ref = value.contiguous(), ref.contiguous()
        out = torch.empty((N, Lq, M * D), dtype=value.dtype, device=value.device)
        loc = torch.empty((N, Lq, M, L, P, 2), dtype=torch.float32, device=value.device)
        attn = torch.empty((N, Lq, M, L, P), dtype=torch.float32, device=value.device)
        with torch.cuda.device(value.device), _timed("fwd_enc"):
            if value.dtype in _H16:
                code = _H16[value.dtype]
                rc = lib().ocpg_msda_fused_fwd_h16(value.data_ptr(), shapes.data_ptr(), level_start.data_ptr(), qproj.data_ptr(), ref.data_ptr(),
                                                   N, S, M, D, L, Lq, P, out.data_ptr(), loc.data_ptr(), attn.data_ptr(), code, stream_ptr())
                if rc == -2000:        # declined, nothing launched: the front end in torch, the un-fused 16-bit forward
                    off, logit = torch.split(qproj.view(N, Lq, -1), [2 * M * L * P, M * L * P], dim=-1)
                    attn = torch.softmax(logit.reshape(N, Lq, M, L * P), -1).view(N, Lq, M, L, P)
                    loc = (ref.view(N, Lq, 1, L, 1, 2) + off.reshape(N, Lq, M, L, P, 2)).contiguous()
                    rc = lib().ocpg_msda_fwd_h16(value.data_ptr(), shapes.data_ptr(), level_start.data_ptr(), loc.data_ptr(), attn.data_ptr(),
                                                 N, S, M, D, L, Lq, P, out.data_ptr(), None, code, stream_ptr())
                check(rc, "ocpg_msda_fused_fwd_h16")
            else:
                check(lib().ocpg_msda_fused_fwd_f32(value.data_ptr(), shapes.data_ptr(), level_start.data_ptr(), qproj.data_ptr(), ref.data_ptr(),
                                                    N, S, M, D, L, Lq, P, out.data_ptr(), loc.data_ptr(), attn.data_ptr(), stream_ptr()),
                      "ocpg_msda_fused_fwd")
        ctx.save_for_backward(value, shapes, level_start, loc, attn)
        ctx.shapes_host = getattr(shapes, "_ocpg_host", None)
        ctx.sel_state = sel_state
        ctx.qshape = qproj.shape
        ctx.mark_non_differentiable(loc, attn)
        return out, loc, attn

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output, _gloc, _gattn):
        value, shapes, level_start, loc, attn = ctx.saved_tensors
        N, S, M, D = value.shape
        _, Lq, _, L, P, _ = loc.shape
        go = grad_output.contiguous()
        hs = ctx.shapes_host if ctx.shapes_host is not None else _host_shapes(shapes)
        if value.dtype in _H16:
            return MSDeformAttnFusedFunction._backward_h16(ctx, value, shapes, level_start, loc, attn, go, hs)
        grad_value = torch.zeros_like(value)
        grad_q = torch.empty(ctx.qshape, dtype=value.dtype, device=value.device)
        L_ = lib()
        with torch.cuda.device(value.device):
            with _timed("bwd_enc_value"):
                args = (loc.data_ptr(), attn.data_ptr(), go.data_ptr(), N, S, M, D, L, Lq, P, grad_value.data_ptr(), ctypes.c_void_p(hs.data_ptr()))
                if ctx.sel_state is not None:
                    rc = L_.ocpg_msda_bwd_value_sel_f32(*args, ctx.sel_state.data_ptr(), stream_ptr())
                else:
                    rc = L_.ocpg_msda_bwd_value_f32(*args, stream_ptr())
            if rc == -2000:        # shape not served by the self-attention scatter kernels: the whole backward through the generic entry point
                grad_value.zero_()
                gl, ga = torch.empty_like(loc), torch.empty_like(attn)
                check(L_.ocpg_msda_bwd_f32(value.data_ptr(), shapes.data_ptr(), level_start.data_ptr(), loc.data_ptr(), attn.data_ptr(), go.data_ptr(),
                                           N, S, M, D, L, Lq, P, grad_value.data_ptr(), gl.data_ptr(), ga.data_ptr(), ctypes.c_void_p(hs.data_ptr()),
                                           stream_ptr()), "ocpg_msda_bwd")
                glogit = attn.view(N, Lq, M, L * P) * (ga.view(N, Lq, M, L * P) - (attn * ga).view(N, Lq, M, L * P).sum(-1, keepdim=True))
                grad_q = torch.cat([gl.reshape(N, Lq, -1), glogit.reshape(N, Lq, -1)], -1)
                return grad_value, None, None, grad_q, None, None, None, None
            check(rc, "ocpg_msda_bwd_value")
            with _timed("bwd_enc_locattn"):
                check(L_.ocpg_msda_fused_bwd_qproj_f32(value.data_ptr(), shapes.data_ptr(), level_start.data_ptr(), loc.data_ptr(), attn.data_ptr(),
                                                       go.data_ptr(), N, S, M, D, L, Lq, P, grad_q.data_ptr(), stream_ptr()), "ocpg_msda_fused_bwd_qproj")
        return grad_value, None, None, grad_q, None, None, None, None

    @staticmethod
    def _backward_h16(ctx, value, shapes, level_start, loc, attn, go, hs):
        """16-bit storage: grad_value from ocpg_msda_bwd_value_h16 (fp32 accumulation, the call site's path selection), grad_qproj from the
        fused gather; when either declines (-2000, nothing launched) the whole backward goes through ocpg_msda_bwd_h16 and the softmax
        backward / concatenation happen in torch, as in the fp32 function."""
        N, S, M, D = value.shape
        _, Lq, _, L, P, _ = loc.shape
        if go.dtype != value.dtype:
            raise RuntimeError(f"MSDeformAttnFusedFunction: grad_output must have value's dtype {value.dtype} (got {go.dtype})")
        code = _H16[value.dtype]
        grad_value = torch.zeros(value.shape, dtype=torch.float32, device=value.device)
        grad_q = torch.empty(ctx.qshape, dtype=torch.float32, device=value.device)
        sel = ctx.sel_state.data_ptr() if ctx.sel_state is not None else None
        hsp = ctypes.c_void_p(hs.data_ptr())
        L_ = lib()
        with torch.cuda.device(value.device):
            with _timed("bwd_enc_value"):
                rc = L_.ocpg_msda_bwd_value_h16(loc.data_ptr(), attn.data_ptr(), go.data_ptr(), N, S, M, D, L, Lq, P, grad_value.data_ptr(), hsp, sel,
                                                code, stream_ptr())
            if rc == 0:
                with _timed("bwd_enc_locattn"):
                    rc = L_.ocpg_msda_fused_bwd_qproj_h16(value.data_ptr(), shapes.data_ptr(), level_start.data_ptr(), loc.data_ptr(), attn.data_ptr(),
                                                          go.data_ptr(), N, S, M, D, L, Lq, P, grad_q.data_ptr(), code, stream_ptr())
                if rc == -2000:
                    grad_value.zero_()         # the scatter has run: start the accumulation over
            if rc == -2000:
                gl, ga = torch.empty_like(loc), torch.empty_like(attn)
                with _timed("bwd_enc"):
                    check(L_.ocpg_msda_bwd_h16(value.data_ptr(), shapes.data_ptr(), level_start.data_ptr(), loc.data_ptr(), attn.data_ptr(), go.data_ptr(),
                                               N, S, M, D, L, Lq, P, grad_value.data_ptr(), gl.data_ptr(), ga.data_ptr(), hsp, sel, code, stream_ptr()),
                          "ocpg_msda_bwd_h16")
                glogit = attn.view(N, Lq, M, L * P) * (ga.view(N, Lq, M, L * P) - (attn * ga).view(N, Lq, M, L * P).sum(-1, keepdim=True))
                grad_q = torch.cat([gl.reshape(N, Lq, -1), glogit.reshape(N, Lq, -1)], -1).view(ctx.qshape)
            else:
                check(rc, "ocpg_msda_fused_bwd_h16")
        return grad_value.to(value.dtype), None, None, grad_q, None, None, None, None


class MSDeformAttnSampleFirstFunction(Function):
    """value_proj + padding fill + the op for calls with FEW queries (cross-attention), float32: the attention-weighted bilinear sample is
    taken from the UNPROJECTED tokens and only the N*Lq*M sampled rows are projected (include/ocpg_hip.h: ocpg_msda_sf_*;
    csrc/msda_sample_first.hip).  Same result as MSDeformAttnFunction on masked_fill(F.linear(src, wv, bv), pad, 0) up to fp32 summation
    order, without the [N*S, C] x [C, C] GEMM, its two backward GEMMs and the dense grad_value.

    apply(src [N,S,C], wv [C,C], bv [C] | None, pad [N,S] bool | None, shapes, level_start, loc [N,Lq,M,L,P,2], attn [N,Lq,M,L,P]) -> out [N,Lq,C]
    `supported()` says whether the kernels serve a call; an unserved call raises here (the module asks first and keeps its old path)."""

    @staticmethod
    def supported(src, wv, bv, loc, attn):
        if not (src.is_cuda and src.dtype == wv.dtype == loc.dtype == attn.dtype == torch.float32 and (bv is None or bv.dtype == torch.float32)):
            return False
        N, S, C = src.shape
        _, Lq, M, L, P, _ = loc.shape
        return C % M == 0 and C % 64 == 0 and C <= 1024 and L * P <= 64 and S * C < 2 ** 31 and N * Lq * M < 2 ** 31

    @staticmethod
    def forward(ctx, src, wv, bv, pad, shapes, level_start, loc, attn):
        for n, t in (("src", src), ("wv", wv), ("shapes", shapes), ("level_start", level_start), ("loc", loc), ("attn", attn)):
            require_gpu(n, t)
        if shapes.dtype != torch.int64 or level_start.dtype != torch.int64:
            raise RuntimeError("MSDeformAttnSampleFirstFunction: spatial_shapes / level_start_index must be int64")
        N, S, C = src.shape
        _, Lq, M, L, P, _ = loc.shape
        D = C // M
        src, wv, loc, attn = src.contiguous(), wv.contiguous(), loc.contiguous(), attn.contiguous()
        bv = None if bv is None else bv.contiguous()
        if pad is not None:
            pad = pad.contiguous()
            pad = pad.view(torch.uint8) if pad.dtype == torch.bool else pad.to(torch.uint8)
        out = torch.empty((N, Lq, C), dtype=torch.float32, device=src.device)
        s = torch.empty((N, Lq, M, C), dtype=torch.float32, device=src.device)
        beta = torch.empty((N, Lq, M), dtype=torch.float32, device=src.device)
        with torch.cuda.device(src.device), _timed("fwd_dec"):
            check(lib().ocpg_msda_sf_fwd_f32(src.data_ptr(), wv.data_ptr(), bv.data_ptr() if bv is not None else None,
                                             pad.data_ptr() if pad is not None else None, shapes.data_ptr(), level_start.data_ptr(),
                                             loc.data_ptr(), attn.data_ptr(), N, S, M, D, L, Lq, P, out.data_ptr(), s.data_ptr(), beta.data_ptr(),
                                             stream_ptr()), "ocpg_msda_sf_fwd_f32")
        ctx.save_for_backward(src, wv, bv, pad, shapes, level_start, loc, attn, s, beta)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        src, wv, bv, pad, shapes, level_start, loc, attn, s, beta = ctx.saved_tensors
        return _sample_first_backward(ctx, grad_output, src, wv, bv, pad, shapes, level_start, loc, attn, s, beta)


def _sample_first_backward(ctx, grad_output, src, wv, bv, pad, shapes, level_start, loc, attn, s, beta):
    """the backward both sample-first functions share; s / beta None: the forward did not run ocpg_msda_sf_fwd_f32, so they are formed here
    (one more launch of that kernel, its `out` dropped) when the weight or bias gradient wants them"""
    N, S, C = src.shape
    _, Lq, M, L, P, _ = loc.shape
    D = C // M
    go = grad_output.contiguous()
    need_src, need_wv, need_bv = ctx.needs_input_grad[0], ctx.needs_input_grad[1], bv is not None and ctx.needs_input_grad[2]
    need_loc, need_attn = ctx.needs_input_grad[6], ctx.needs_input_grad[7]
    grad_src = grad_loc = grad_attn = grad_wv = grad_bv = None
    p = lambda t: t.data_ptr() if t is not None else None      # noqa: E731
    with torch.cuda.device(src.device), _timed("bwd_dec"):
        if need_src or need_loc or need_attn:
            grad_src = torch.zeros_like(src) if need_src else None
            grad_loc, grad_attn = torch.empty_like(loc), torch.empty_like(attn)
            check(lib().ocpg_msda_sf_bwd_f32(src.data_ptr(), wv.data_ptr(), p(bv), p(pad), shapes.data_ptr(), level_start.data_ptr(),
                                             loc.data_ptr(), attn.data_ptr(), go.data_ptr(), N, S, M, D, L, Lq, P,
                                             p(grad_src), grad_loc.data_ptr(), grad_attn.data_ptr(), stream_ptr()), "ocpg_msda_sf_bwd_f32")
        if need_wv or need_bv:
            if s is None:
                out = torch.empty((N, Lq, C), dtype=torch.float32, device=src.device)
                s = torch.empty((N, Lq, M, C), dtype=torch.float32, device=src.device)
                beta = torch.empty((N, Lq, M), dtype=torch.float32, device=src.device)
                check(lib().ocpg_msda_sf_fwd_f32(src.data_ptr(), wv.data_ptr(), p(bv), p(pad), shapes.data_ptr(), level_start.data_ptr(),
                                                 loc.data_ptr(), attn.data_ptr(), N, S, M, D, L, Lq, P, out.data_ptr(), s.data_ptr(),
                                                 beta.data_ptr(), stream_ptr()), "ocpg_msda_sf_fwd_f32")
            grad_wv = torch.empty_like(wv)
            grad_bv = torch.empty_like(bv) if need_bv else None
            check(lib().ocpg_msda_sf_bwd_params_f32(go.data_ptr(), s.data_ptr(), beta.data_ptr(), N, M, D, Lq, grad_wv.data_ptr(),
                                                    p(grad_bv), stream_ptr()), "ocpg_msda_sf_bwd_params_f32")
    return (grad_src, grad_wv if need_wv else None, grad_bv, None, None, None, grad_loc if need_loc else None,
            grad_attn if need_attn else None)


class MSDeformAttnSampleFirstBackwardFunction(Function):
    """Same inputs, same result and same gradients as MSDeformAttnSampleFirstFunction, but the FORWARD keeps today's order -- value_proj over
    all N*S tokens (the module's own Linear routing), the padding fill, ocpg_msda_fwd_f32 -- so `out` has today's bits; `value` is dropped
    right after (it is not saved), and the backward is the sample-first one: no dense grad_value, none of value_proj's two backward GEMMs.
    Why: under bf16 autocast a change in the last fp32 bits of the decoder's cross-attention output moves the step's outputs by whole
    bf16 roundings, so the default keeps them and takes the backward's share of the gain.
    Call it with gradients enabled (the module does): without them there is no backward to save anything in."""

    supported = staticmethod(MSDeformAttnSampleFirstFunction.supported)

    @staticmethod
    def forward(ctx, src, wv, bv, pad, shapes, level_start, loc, attn):
        from ...amp_cache import linear
        for n, t in (("src", src), ("wv", wv), ("shapes", shapes), ("level_start", level_start), ("loc", loc), ("attn", attn)):
            require_gpu(n, t)
        N, S, C = src.shape
        M = loc.shape[2]
        src, wv, loc, attn = src.contiguous(), wv.contiguous(), loc.contiguous(), attn.contiguous()
        bv = None if bv is None else bv.contiguous()
        with torch.enable_grad():        # the routing of `linear` (which GEMM serves value_proj) looks at the grad mode and at wv.requires_grad
            value = linear(src.detach(), wv, bv).detach()
        if pad is not None:
            value = value.masked_fill(pad[..., None], 0.0)
            pad = pad.contiguous()
            pad = pad.view(torch.uint8) if pad.dtype == torch.bool else pad.to(torch.uint8)
        out = ms_deform_attn_forward(value.view(N, S, M, C // M), shapes, level_start, loc, attn)
        ctx.save_for_backward(src, wv, bv, pad, shapes, level_start, loc, attn)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        return _sample_first_backward(ctx, grad_output, *ctx.saved_tensors, None, None)
